"""Cases and the plain restatement of the tokens of `tokens --gaps-bed`, shared by the CPU and the GPU tests.

A BED row "name \\t a \\t b" stands for what `samtools faidx REF name:a-b` prints: the header "name:a-b" from the literal text of the fields, the bases
[max(a, 1) - 1, min(b, contig length)).  rows() reads a BED that way, tokens() tiles the regions as gaps_to_fasta.py tiles the sequences of GAPS.fa
(range(R, len, S)), qname_hash() is the fork's fragment hash (X31 over the name, the two Wang terms), gaps_fasta() writes the equivalent GAPS.fa."""
import bisect
import random

M = 0xffffffff


def wang(k):
    k = (k + (~(k << 15) & M)) & M; k ^= k >> 10; k = (k + (k << 3)) & M; k ^= k >> 6; k = (k + (~(k << 11) & M)) & M; k ^= k >> 16
    return k


def x31(s):
    h = s[0]
    for c in s[1:]:
        h = (h * 31 + c) & M
    return h


def qname_hash(name, qlen, seed):
    return wang(x31(name) ^ ((wang(qlen & M) + wang(seed & M)) & M))


class BedError(Exception):
    def __init__(self, line, why):
        Exception.__init__(self, "line %d: %s" % (line, why)); self.line = line


def rows(bed, contigs):
    """[(head, contig index, start, length)] of the rows of the BED text (bytes); contigs: [(name, length)].  Raises BedError with the 1-based line."""
    out = []
    for n, l in enumerate(bed.split(b"\n"), 1):
        l = l.rstrip(b"\r")
        if not l:
            continue
        f = l.split(b"\t")
        if len(f) < 3:
            raise BedError(n, "fields")
        if not (f[1].isdigit() and f[2].isdigit() and f[1].isascii() and f[2].isascii()):
            raise BedError(n, "number")
        a, b = int(f[1]), int(f[2])
        if b < a:
            raise BedError(n, "order")
        idx = [i for i, (nm, _) in enumerate(contigs) if nm == f[0]]
        if not idx:
            raise BedError(n, "contig")
        s, e = max(a, 1) - 1, min(b, contigs[idx[0]][1])
        s = min(s, e)
        out.append((f[0] + b":" + f[1] + b"-" + f[2], idx[0], s, e - s))
    return out


def tokens(lens, R, S):
    """[(row, offset)] in order: range(R, len, S) of every row"""
    return [(r, k * S) for r, n in enumerate(lens) for k in range(len(range(R, n, S)))]


def table(heads, lens, R, S):
    first = [0]
    for n in lens:
        first.append(first[-1] + len(range(R, n, S)))
    return first, [x31(h + b"_") for h in heads]


def expected(heads, src, lens, R, S, seed):
    """(first_tok, h_prefix, [(start, hash)] of every token, [row of every token])"""
    first, hp = table(heads, lens, R, S)
    tk = tokens(lens, R, S)
    return first, hp, [(src[r] + o, qname_hash(heads[r] + b"_%d" % o, R, seed)) for r, o in tk], [r for r, _ in tk]


def runs(first, t0, n):
    """[(first token relative to t0, row)] of the rows that own tokens [t0, t0 + n)"""
    out = []
    r = max(bisect.bisect_left(first, t0) - 1, 0)          # every row before it ends at or before t0
    while r < len(first) - 1 and first[r] < t0 + n:
        lo, hi = max(first[r], t0), min(first[r + 1], t0 + n)
        if lo < hi:
            out.append((lo - t0, r))
        r += 1
    return out


def gaps_fasta(bed, seqs):
    """The GAPS.fa that extract_fasta_regions_with_bedfile.sh makes of the BED: per row `samtools faidx`'s record, 60 bases per line.  seqs: [(name, str)]."""
    out = []
    for head, c, s, n in rows(bed, [(nm, len(q)) for nm, q in seqs]):
        q = seqs[c][1][s:s + n]
        out.append(b">" + head + b"\n" + b"".join(q[i:i + 60].encode() + b"\n" for i in range(0, len(q), 60)))
    return b"".join(out)


def gap_names(bed):
    return [b":".join((f[0], b"-".join(f[1:3]))) for f in (l.rstrip(b"\r").split(b"\t") for l in bed.split(b"\n")) if len(f) >= 3]


def row(c, start, n):
    """the BED line of contig c's bases [start, start + n), n > 0"""
    return b"%s\t%d\t%d" % (c, start + 1, start + n)


CONTIGS = [(b"c2", 12000), (b"cA", 8000), (b"c10", 9000)]          # the `planted` lengths
R0, S0 = 100, 7


def _bed_case(name, R, S, lines, contigs=CONTIGS, seed=11):
    off = [0]
    for _, n in contigs:
        off.append(off[-1] + n)
    rr = rows(b"\n".join(lines) + b"\n", contigs)
    return dict(name=name, R=R, S=S, seed=seed, heads=[h for h, _, _, _ in rr], src=[off[c] + s for _, c, s, _ in rr], lens=[n for _, _, _, n in rr], bed=lines, contigs=contigs)


def _big():
    rnd = random.Random(20261019); lines = []
    for _ in range(900):
        c, cl = CONTIGS[rnd.randrange(3)]
        n = rnd.choice([0, 50, 99, 100, 101, 107, 108, 400, 1500, 2500])
        s = rnd.randrange(0, cl - n)
        lines.append(b"%s\t%d\t%d" % (c, s + 1, s + n) if n else b"%s\t%d\t%d" % (c, s + 5, s + 5))
    return lines


def cases():
    """Dicts name, R, S, seed, heads, src, lens (and bed, contigs where the table is a BED's)."""
    R, S = R0, S0
    zero = [row(b"cA", 10, 50), row(b"cA", 20, R), row(b"c10", 0, 1)]
    c = [_bed_case("lengths", R, S, [row(b"c2", 1000 + 300 * i, n) for i, n in enumerate((R - 1, R, R + 1, R + S, R + S + 1))]),
         _bed_case("a0_a1", R, S, [b"c2\t0\t300", b"c2\t1\t300"]),
         _bed_case("b_beyond", R, S, [b"cA\t7800\t99999", b"c10\t8850\t4000000000000"]),
         _bed_case("last_R1", R, S, [row(b"c10", 9000 - (R + 1), R + 1), row(b"c2", 12000 - (R + 1), R + 1)]),
         _bed_case("zero_runs", R, S, zero + [row(b"c2", 500, 300)] + zero[:2] + [row(b"cA", 100, R + 1)] + zero + zero[:1]),
         _bed_case("only_zero", R, S, zero),
         _bed_case("same_twice", R, S, [row(b"cA", 3000, 250)] * 2),
         _bed_case("S1", 10, 1, [row(b"c2", 77, 300), row(b"c10", 8700, 300)]),
         _bed_case("leading_zeros", R, S, [b"c2\t007\t300", b"c2\t7\t0300"]),
         _bed_case("extra_columns_crlf", R, S, [b"c2\t100\t400\tx\t0\t+\r", b"", b"cA\t1\t200\t"]),
         _bed_case("start_and_7", R, 20, [row(b"c2", 8 * 100 + i, 160 + i) for i in range(8)] + [row(b"c10", 9000 - 150, 150)]),
         _bed_case("big", R, S, _big()),
         # k * S at every number of digits from 1 to 7 (the three tables together)
         dict(name="digits_1_5_6", R=100, S=99991, seed=11, heads=[b"chr1:5000001-6100000"], src=[5000000], lens=[1100000]),
         dict(name="digits_1_4_5_6_7", R=100, S=1099, seed=11, heads=[b"chr1:1-1100000"], src=[0], lens=[1100000]),
         dict(name="digits_1_2_3_4", R=100, S=33, seed=0, heads=[b"x:1-1500"], src=[123456789], lens=[1500]),
         # windows on either side of 2^32 in the concatenated reference, and one token that starts below and ends above
         dict(name="src_2_32", R=100, S=7, seed=-5, heads=[b"chr9:1-400", b"chr9:500-900", b"chrX:1-200"], src=[2 ** 32 - 250, 2 ** 32 + 5, 2 ** 33 + 1], lens=[400, 401, 200])]
    return c


def ranges(first):
    """(t0, n) of the launches the kernel test makes: everything, one token, a launch inside one row, one from a row's first token to inside the next row
    that has tokens (across the rows without tokens between them), one that ends on a row's last token"""
    n_tok = first[-1]
    if n_tok == 0:
        return [(0, 0)]
    out = [(0, n_tok), (n_tok - 1, 1)]
    own = [r for r in range(len(first) - 1) if first[r + 1] > first[r]]
    r = own[0]
    if first[r + 1] - first[r] >= 3:
        out.append((first[r] + 1, first[r + 1] - first[r] - 2))
    if len(own) > 1:
        a, b = own[0], own[1]
        out.append((first[a], first[b] - first[a] + 1))
        out.append((first[a + 1] - 1, first[b + 1] - first[a + 1] + 1))
        a, b = own[-2], own[-1]
        out.append((first[a] + (first[a + 1] - first[a]) // 2, first[b + 1] - first[a] - (first[a + 1] - first[a]) // 2))
    return sorted(set(out))


MALFORMED = [(b"c2\t1\t300\nc2\t5\n", 2), (b"c2 1 300\n", 1), (b"\nc2\tx\t300\n", 2), (b"c2\t1\t3e2\n", 1), (b"c2\t1\t\n", 1), (b"c2\t-1\t300\n", 1),
             (b"c2\t1\t300\n\n\nc2\t300\t299\n", 4), (b"c2\t1\t300\nc3\t1\t300\n", 2), (b"c2\t1\t300\r\n\tc2\t1\t300\n", 2), (b"c2\t 1\t300\n", 1)]


def ref_code(p):
    """the base code of place p of the sanitizer program's synthetic reference"""
    return (p * 7 + p // 13) % 5

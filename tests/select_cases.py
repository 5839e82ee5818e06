"""Case texts of the --gpu-select tests (test_select_cpu.py, test_select_san_cpu.py, test_gpu_select.py): pairs of FASTQ texts with the names to select,
built from a fixed seed, and what each case expects of the run besides equal output -- how many records of each file the default reader is handed.

The hand-over counts follow from the kseq grammar of the default reader (al_seqio.h):
  * a regular file hands over nothing; a trailing blank line leaves a rest that holds no record: 0;
  * a multi-line record is ONE record of the default reader: it and everything behind it is handed over;
  * '@' or '>' at the start of a sequence line ends the sequence: the reader delivers the record with an empty sequence, takes the line for the next
    header, finds '+', a quality line that is longer than the (empty) sequence, and ends the input: 1 record handed over;
  * '+' at the start of a sequence line is taken for the separator; the next line ('+') is a quality of one byte for an empty sequence: the input ends
    before any record is delivered: 0;
  * a FASTA file is the default reader's from byte 0: all of its records."""
import collections
import random

import inflate_cases as ic

Case = collections.namedtuple("Case", "name fq l1 l2 handed oracle")   # fq: two texts; l1 / l2: names; handed: records per file; oracle: plain four-line input

DIRECTED_LENS = [1, 3, 4, 5, 63, 64, 65, 254]


def _rec(rng, name, n=None, comment=b"", eol=b"\n", bases=b"ACGT"):
    n = rng.randrange(100, 151) if n is None else n
    seq = bytes(rng.choice(bases) for _ in range(n)); qual = bytes(rng.randrange(35, 74) for _ in range(n))
    return b"@" + name + comment + eol + seq + eol + b"+" + eol + qual + eol


def _name_of_len(k, tag):
    s = (tag + b"x" * k)[:k]
    return s


def base_pair(seed=5, n=600):
    """About n records per file: random reads with the directed names in between.  Returns (text1, text2, names1, names2)."""
    rng = random.Random(seed)
    names = [b"read%d" % i for i in range(n)]
    directed = [_name_of_len(k, b"L%d_" % k) for k in DIRECTED_LENS] + [b"r1", b"r10", b"r1/1"]
    pos = sorted(rng.sample(range(5, n - 5), len(directed)))
    for p, d in zip(pos, directed):
        names[p] = d
    names[300] = names[200]                                        # the same name twice in one file: both records are kept, in order
    t = []
    for f in (0, 1):
        recs = []
        for i, nm in enumerate(names):
            cm = b" 1:N:0" if (i % 7 == 0 and f == 0) else b"\tcomment" if i % 11 == 0 else b""
            recs.append(_rec(rng, nm, 5000 if i == 150 else None, cm))          # one record of 5 000 bases: longer than the smallest pieces
        t.append(b"".join(recs))
    sel = set(directed) | {names[0], names[n - 1], names[150], names[200]} | set(rng.sample(names, n // 20))
    l1 = sorted(sel | {b"in_no_file", b"only_in_l1"})
    l2 = sorted(sel - {b"r10"} | {b"in_no_file"})
    # a name that is only in l1 but occurs in file 2 (and not in file 1)
    t[1] += _rec(rng, b"only_in_l1")
    t[0] += _rec(rng, b"tail_of_1")
    return t[0], t[1], l1, l2


def _names_in(text):
    return [l[1:].split()[0] if len(l) > 1 and l[1:].split() else b"" for l in text.split(b"\n")[0::4] if l.startswith(b"@")]


def _small(rng, n, **kw):
    return [_rec(rng, b"s%d" % i, rng.randrange(20, 60), **kw) for i in range(n)]


def cases():
    rng = random.Random(17)
    t1, t2, l1, l2 = base_pair()
    every = sorted(set(_names_in(t1)) | set(_names_in(t2)))
    out = [Case("base", (t1, t2), l1, l2, (0, 0), True),
           Case("none", (t1, t2), [], [], (0, 0), True),
           Case("all", (t1, t2), every, every, (0, 0), True),
           Case("probe5000", (t1, t2), sorted(set(l1) | {b"n%05d" % i for i in range(5000)}), sorted(set(l2) | {b"m%05d" % i for i in range(5000)}), (0, 0), True)]
    a = _small(rng, 12); b = _small(rng, 12)
    a[5] = b"@s5\n\n+\n\n"                                        # an empty sequence
    sel = [b"s0", b"s5", b"s7", b"s11"]
    out.append(Case("empty_seq", (b"".join(a), b"".join(b)), sel, sel, (0, 0), True))
    a = _small(rng, 12, bases=b"ACGTuUNn"); b = _small(rng, 12, bases=b"ACGUu")
    out.append(Case("u_bases", (b"".join(a), b"".join(b)), sel, sel, (0, 0), False))
    a = _small(rng, 12, eol=b"\r\n"); b = _small(rng, 12)
    a[5] = b"@s5 c\r\n\r\n+\r\n\r\n"
    out.append(Case("crlf", (b"".join(a), b"".join(b)), sel, sel, (0, 0), False))
    a = _small(rng, 12); b = _small(rng, 12)
    out.append(Case("unterminated", (b"".join(a)[:-1], b"".join(b)[:-1]), sel, sel, (0, 0), True))
    out.append(Case("trailing_blank", (b"".join(a) + b"\n", b"".join(b)), sel, sel, (0, 0), True))
    # irregular records in file 1, at record 6 of 12; file 2 stays regular
    ml = _small(rng, 12)
    ml[6] = b"@s6\nACGTACGT\nACGTAC\n+\nIIIIIIII\nIIIIII\n"
    out.append(Case("multiline", (b"".join(ml), b"".join(b)), sel + [b"s6"], sel, (6, 0), False))
    for nm, ch, handed in (("seq_at", b"@", 1), ("seq_plus", b"+", 0), ("seq_gt", b">", 1)):
        x = _small(rng, 12)
        x[6] = b"@s6\n" + ch + b"ACGTACG\n+\nIIIIIIII\n"
        out.append(Case(nm, (b"".join(x), b"".join(b)), sel + [b"s6"], sel, (handed, 0), False))
    fa = b"".join(b">s%d\n%s\n" % (i, bytes(rng.choice(b"ACGT") for _ in range(40))) for i in range(12))
    out.append(Case("fasta", (fa, fa), sel, sel, (12, 12), False))
    return out


def rows(l1, l2):
    """The rows file extract-sequence reads: column 4 is the name with .1 / .2."""
    return b"".join(b"chr1\t0\t1\t%s.%d\t60\t*\n" % (n, k) for k, l in ((1, l1), (2, l2)) for n in l)


def tap_text(n_rec, seed=3):
    """A text of exactly n_rec regular records and a list of names that selects about a third of them."""
    rng = random.Random(seed * 1000 + n_rec)
    names = [b"t%d" % i for i in range(n_rec)]
    text = b"".join(_rec(rng, nm, rng.randrange(1, 90)) for nm in names)
    return text, sorted(rng.sample(names, n_rec // 3)) + [b"absent"]


def bgzf(blob, block, eof=True):
    return b"".join(ic.member(ic.deflate_raw(blob[o:o + block], 6), blob[o:o + block]) for o in range(0, len(blob), block)) + (ic.EOF_BLOCK if eof else b"")

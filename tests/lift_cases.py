"""The rules of `airlift-align lift` (airlift_amd/csrc/al_dev_lift.h) restated in Python, independent of the C++: the block table as sorted lists searched with
bisect, the lift of an interval, the per-record rules, the header.  And the directed inputs of the lift's tests: a chain file with every kind of block, BAMs of
0 .. 257 records that meet every rule, the shapes that aim at the edges of k_bam_walk's window, and the malformed inputs.

The BAMs are built here (rec_bytes / bam_bytes, compressed with select_cases.bgzf), not with write_bam of test_extract_cpu.py: that writer makes plain gzip
members without the BC subfield, which `lift` refuses by design (it reads a BAM by its BGZF members), and its records have no mate fields, tags or bin to
set.  write_bam is used where its output is the point: the refusal of a file that is gzip but not BGZF (test_lift_cpu.py)."""
import bisect
import struct

from select_cases import bgzf

CIG = "MIDNSHP=X"
KEPT, UNLIFTED, UNMAPPED = 0, 1, 2


# ---- the rules -----------------------------------------------------------------------------------------------------------------------------------------
class Table:
    """chain file text -> per tName the blocks (tStart, size, qSlot, qStart, minus) sorted by (tStart, file index), their starts and prefix maxima of the ends"""

    def __init__(self, text):
        self.q_names, self.q_sizes, self.t_size, self.blocks = [], [], {}, {}
        t = q = 0
        for line in text.split("\n"):
            f = line.split()
            if not f or line.startswith("#"):
                continue
            if f[0] == "chain":
                tname, tsize, tstart, qname, qsize, qstrand, qstart = f[2], int(f[3]), int(f[5]), f[7], int(f[8]), f[9], int(f[10])
                self.t_size.setdefault(tname, tsize)
                if qname not in self.q_names:
                    self.q_names.append(qname); self.q_sizes.append(qsize)
                cur = (tname, self.q_names.index(qname), qstrand == "-")
                t, q = tstart, qstart
                continue
            size = int(f[0]); dt, dq = (int(f[1]), int(f[2])) if len(f) == 3 else (0, 0)
            self.blocks.setdefault(cur[0], []).append((t, size, cur[1], q, cur[2]))
            t += size + dt; q += size + dq
        self.starts, self.pmax = {}, {}
        for name, b in self.blocks.items():
            b.sort(key=lambda x: x[0])            # (stable: file order among equal starts)
            self.starts[name] = [x[0] for x in b]
            m, pm = 0, []
            for x in b:
                m = max(m, x[0] + x[1]); pm.append(m)
            self.pmax[name] = pm

    def lift(self, chrom, s, e):
        """(qSlot, d) or None"""
        b = self.blocks.get(chrom)
        if not b:
            return None
        i = bisect.bisect_right(self.starts[chrom], s) - 1
        if i < 0:
            return None
        tstart, size, qslot, qstart, minus = b[i]
        if e > tstart + size or (i > 0 and self.pmax[chrom][i - 1] > s) or (i + 1 < len(b) and b[i + 1][0] < e) or minus:
            return None
        return qslot, qstart - tstart


def reg2bin(beg, end):
    end -= 1
    for sh, off in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> sh == end >> sh:
            return (off + (beg >> sh)) & 0xffff
    return 0


def i32(v):
    v &= 0xffffffff
    return v - (1 << 32) if v >> 31 else v


def lift_record(tab, refs, r):
    """r: a record dict (rid, pos, mapq, flag, cig, qname, nrid, npos, tlen, bin, ...) -> (verdict, the kept record or None, the BED row or None)"""
    reflen = sum(l for l, o in r["cig"] if o in "MDN=X") or 1
    chrom = refs[r["rid"]][0] if r["rid"] >= 0 else None
    o = dict(r); q_own, d_own = -1, 0
    if not r["flag"] & 4 and r["rid"] >= 0:
        hit = tab.lift(chrom, r["pos"], r["pos"] + reflen)
        if hit is None:
            name = r["qname"] + (".1" if r["flag"] & 64 else ".2" if r["flag"] & 128 else "")
            cs = "".join("%d%s" % c for c in r["cig"]) or "*"
            return UNLIFTED, None, "%s\t%d\t%d\t%s\t%d\t%s" % (chrom, r["pos"], r["pos"] + reflen, name, r["mapq"], cs)
        q_own, d_own = hit
        o["rid"], o["pos"] = q_own, r["pos"] + d_own; o["bin"] = reg2bin(o["pos"], o["pos"] + reflen)
        verdict = KEPT
    else:
        verdict = UNMAPPED
        if r["flag"] & 4 and r["rid"] >= 0:
            hit = tab.lift(chrom, r["pos"], r["pos"] + 1)
            if hit is None:
                o["rid"], o["pos"], o["bin"] = -1, -1, 4680
            else:
                q_own, d_own = hit
                o["rid"], o["pos"] = q_own, r["pos"] + d_own; o["bin"] = reg2bin(o["pos"], o["pos"] + 1)
    if r["flag"] & 1 and not r["flag"] & 8 and r["nrid"] >= 0:
        hit = tab.lift(refs[r["nrid"]][0], r["npos"], r["npos"] + 1)
        if hit is None:
            o["nrid"], o["npos"], o["tlen"] = -1, -1, 0
            o["flag"] = (r["flag"] | 8) & ~0x22
        else:
            o["nrid"], o["npos"] = hit[0], r["npos"] + hit[1]
            o["tlen"] = i32(r["tlen"] + hit[1] - d_own) if hit[0] == q_own and r["tlen"] != 0 else 0
    return verdict, o, None


def lift_all(chain_text, refs, recs):
    """-> verdicts, kept records (dicts, in input order), BED rows (in input order)"""
    tab = Table(chain_text)
    for name, ln in refs:
        assert name not in tab.t_size or tab.t_size[name] == ln
    v, kept, rows = [], [], []
    for r in recs:
        a, k, row = lift_record(tab, refs, r)
        v.append(a)
        if k is not None:
            kept.append(k)
        if row is not None:
            rows.append(row)
    return v, kept, rows


def lift_header(text, tab):
    """the header text of the lifted BAM"""
    lines = text.split("\n"); last = lines.pop()           # (last: what follows the last newline, kept as it is)
    sq = ["@SQ\tSN:%s\tLN:%d" % x for x in zip(tab.q_names, tab.q_sizes)]
    is_ = lambda l, t: l[:3] == t and (len(l) == 3 or l[3] == "\t")
    if last:
        lines.append(last)
    any_sq = any(is_(l, "@SQ") for l in lines)
    out, put = [], False
    if not any_sq and not (lines and is_(lines[0], "@HD")):
        out += sq; put = True
    for i, l in enumerate(lines):
        if is_(l, "@SQ"):
            if not put:
                out += sq; put = True
            continue
        if is_(l, "@HD"):
            l = "\t".join("SO:unsorted" if f[:3] == "SO:" else f for f in l.split("\t"))
        out.append(l)
        if not put and not any_sq and i == 0:
            out += sq; put = True
    return "".join(x + "\n" for x in out)


# ---- BAM bytes --------------------------------------------------------------------------------------------------------------------------------------------
def rec(rid, pos, flag=0, cig=((100, "M"),), qname="r", mapq=30, nrid=-1, npos=-1, tlen=0, l_seq=0, tags=b"", bin_=4680):
    return dict(rid=rid, pos=pos, mapq=mapq, flag=flag, cig=list(cig), qname=qname, nrid=nrid, npos=npos, tlen=tlen, l_seq=l_seq, tags=tags, bin=bin_)


def rec_bytes(r):
    body = struct.pack("<iiBBHHHiiii", r["rid"], r["pos"], len(r["qname"]) + 1, r["mapq"], r["bin"], len(r["cig"]), r["flag"], r["l_seq"], r["nrid"], r["npos"], r["tlen"])
    body += r["qname"].encode() + b"\0" + b"".join(struct.pack("<I", l << 4 | CIG.index(o)) for l, o in r["cig"])
    body += b"\x12" * ((r["l_seq"] + 1) // 2) + b"\x1e" * r["l_seq"] + r["tags"]
    return struct.pack("<i", len(body)) + body


def header_bytes(text, refs):
    t = text.encode()
    return b"BAM\1" + struct.pack("<i", len(t)) + t + struct.pack("<i", len(refs)) + b"".join(struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l) for n, l in refs)


def bam_bytes(text, refs, recs):
    return header_bytes(text, refs) + b"".join(rec_bytes(r) for r in recs)


def bgzf_at(blob, cuts):
    """BGZF with members that end exactly at the offsets `cuts` (and every 0xff00 bytes in between)"""
    out, a = [], 0
    for c in sorted(set(cuts)) + [len(blob)]:
        if c > a:
            out.append(bgzf(blob[a:c], 0xff00, eof=False)); a = c
    return b"".join(out) + bgzf(b"", 0xff00)


def sized_rec(total, rid=0, pos=500, qname="s"):
    """a record of exactly `total` bytes (block_size field included), total >= 42 + len(qname)"""
    base = 4 + 32 + len(qname) + 1 + 4
    pad = total - base
    assert pad == 0 or pad >= 4, total
    return rec(rid, pos, qname=qname, tags=b"" if pad == 0 else b"XZZ" + b"x" * (pad - 4) + b"\0")


# ---- the directed inputs ------------------------------------------------------------------------------------------------------------------------------------
CHAIN = """chain 1000 chrA 10000 + 100 5000 newA 12000 + 300 5250 1
1000 100 200
900 50 0
2850

chain 500 chrA 10000 + 4000 4500 newB 3000 + 0 500 2
500

chain 300 chrB 8000 + 1000 3000 newA 12000 - 6000 8000 3
2000

chain 200 chrB 8000 + 4000 6000 newB 3000 + 1000 3000 4
2000

chain 100 chrD 500 + 0 500 newC 700 + 100 600 5
500
"""
REFS = [("chrA", 10000), ("chrB", 8000), ("chrC", 5000)]
HEADER = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chrA\tLN:10000\n@SQ\tSN:chrB\tLN:8000\n@SQ\tSN:chrC\tLN:5000\n@PG\tID:x\tPN:x\n"
HEADERS = {"full": HEADER, "hd_only": "@HD\tVN:1.6\tSO:queryname\tGO:none\n@PG\tID:x\n", "pg_only": "@PG\tID:x\n@CO\tno SQ and no HD\n", "empty": "",
           "sq_first": "@SQ\tSN:chrA\tLN:10000\n@HD\tVN:1.6\n@SQ\tSN:chrB\tLN:8000\n@RG\tID:g\n@SQ\tSN:chrC\tLN:5000\n"}

NM = b"NMi\x03\x00\x00\x00"
POOL = [
    rec(0, 500),                                                   # wholly in block 0 (d = 200)
    rec(0, 100), rec(0, 1000), rec(0, 99), rec(0, 1001),           # touching each edge, and over it by one base
    rec(0, 1050, cig=[(200, "M")]),                                # spanning a gap
    rec(0, 1200), rec(0, 2000), rec(0, 2001),                      # block 1 (d = 300): its first base, its last, one over
    rec(0, 4100), rec(0, 3950), rec(0, 4600),                      # in two overlapping blocks of different chains; across the second one's start; behind it
    rec(2, 500), rec(1, 100),                                      # a contig the chain lacks; a contig of the chain, outside every block
    rec(0, 600, cig=[]), rec(0, 1150, cig=[]), rec(0, 700, cig=[(50, "S"), (50, "I")]),   # reflen 0: a point
    rec(0, 300, cig=[(5, "H"), (10, "S"), (40, "M"), (3, "D"), (20, "M"), (100, "N"), (30, "M"), (2, "I"), (10, "S")], tags=NM),
    rec(0, 950, cig=[(40, "="), (3, "D"), (20, "X"), (100, "N"), (30, "M")]),             # reflen 193: over block 0's end
    rec(0, 500, 1 | 2 | 32 | 64, nrid=0, npos=700, tlen=300, qname="pairA"), rec(0, 700, 1 | 2 | 16 | 128, nrid=0, npos=500, tlen=-300, qname="pairA"),
    rec(0, 500, 1 | 2 | 32 | 64, nrid=0, npos=1300, tlen=900, qname="pairB"), rec(0, 1300, 1 | 2 | 16 | 128, nrid=0, npos=500, tlen=-900, qname="pairB", tags=NM),   # two blocks, d = 200 and 300
    rec(0, 500, 1 | 2 | 32 | 64, nrid=0, npos=1120, tlen=720, qname="pairC"), rec(0, 1120, 1 | 2 | 16 | 128, nrid=0, npos=500, tlen=-720, qname="pairC"),           # the second mate does not lift
    rec(0, 500, 1 | 64, nrid=1, npos=4500, tlen=0, qname="pairD"), rec(1, 4500, 1 | 128, nrid=0, npos=500, tlen=0, qname="pairD"),                                  # mates on two contigs
    rec(0, 500, 1 | 8 | 64, nrid=0, npos=500, qname="pairE"), rec(0, 500, 4 | 1 | 128, nrid=0, npos=500, qname="pairE"),                                          # a mapped read and its unmapped mate, placed
    rec(0, 1150, 4 | 1 | 64, nrid=0, npos=1150, qname="pairF"), rec(-1, -1, 4 | 1 | 8 | 64, qname="pairG"), rec(-1, -1, 4, qname="lone"),                          # unmapped: placed in a gap; without placement
    rec(0, 2200, 256), rec(0, 2200, 2048 | 16, tags=b"SAZchrA,1,+,100M,0,0;\0"),                                                                                    # secondary, supplementary
    rec(1, 1500), rec(1, 4100), rec(1, 5950),                      # a '-' chain's block; a '+' chain's on the same contig; over its end
    rec(0, 500, 1 | 64, nrid=1, npos=1500, tlen=0, qname="pairH"),                                                                                                  # the mate lies in a '-' block
    rec(0, 2500, 1 | 2 | 64, nrid=0, npos=2700, tlen=0, qname="pairI"),                                                                                             # tlen 0 stays 0
    rec(0, -1), rec(-1, 500), rec(0, 4999, cig=[(1, "M")]), rec(0, 4999, cig=[(2, "M")]),                                                                          # pos -1; no refID and no flag 4; the last base
]


def directed(n):
    """n records: the pool in order, again and again, with names of every length from 1 to 40"""
    out = []
    for k in range(n):
        r = dict(POOL[k % len(POOL)])
        if r["qname"] == "r":
            r["qname"] = ("q%d" % k).ljust(1 + k % 40, "x")
        else:
            r["qname"] = "%s_%d" % (r["qname"], k // len(POOL))
        out.append(r)
    return out


SIZES = (0, 1, 63, 64, 65, 257)


def walk_sets(W):
    """name -> records whose stream (behind HEADER / REFS) aims at the window size W of k_bam_walk: a block_size field cut by a window's edge after 1, 2
    and 3 bytes, a record longer than 2 W, and a record that ends exactly at an edge"""
    h = len(header_bytes(HEADER, REFS)); out = {}
    for cut in (0, 1, 2, 3):
        recs = directed(20); used = h + sum(len(rec_bytes(r)) for r in recs)
        recs.append(sized_rec(2 * W - cut - used, qname="fill"))      # the next record's block_size starts `cut` bytes in front of offset 2 W
        recs += directed(30)
        out["cut%d" % cut] = recs
    out["long"] = directed(5) + [sized_rec(2 * W + 777, qname="long")] + directed(9) + [sized_rec(5 * W + 1, pos=1050, qname="longer")] + directed(3)
    return out


def malformed():
    """name -> (uncompressed BAM bytes, what the message must say)"""
    good = directed(40); h = header_bytes(HEADER, REFS); out = {}
    def stream(k, bad):
        return h + b"".join(rec_bytes(r) for r in good[:k]) + bad + b"".join(rec_bytes(r) for r in good[k:])
    b = bytearray(rec_bytes(good[7])); off7 = len(h) + sum(len(rec_bytes(r)) for r in good[:7])
    out["size31"] = (stream(7, struct.pack("<i", 31) + b"\0" * 31), "offset %d of the inflated stream: block_size below 32" % off7)
    out["size_big"] = (stream(7, struct.pack("<i", (1 << 28) + 1) + bytes(b[4:])), "offset %d of the inflated stream: block_size below 32" % off7)
    out["size_negative"] = (stream(7, struct.pack("<i", -5) + bytes(b[4:])), "offset %d of the inflated stream: block_size below 32" % off7)
    x = bytearray(b); x[4 + 32 + x[12] - 1] = ord("z"); out["no_nul"] = (stream(7, bytes(x)), "offset %d of the inflated stream: the name is not NUL-terminated" % off7)
    x = bytearray(b); struct.pack_into("<H", x, 16, 60000); out["cigar_beyond"] = (stream(7, bytes(x)), "offset %d of the inflated stream: the name and the CIGAR do not fit" % off7)
    x = bytearray(b); x[12] = 0; out["name0"] = (stream(7, bytes(x)), "offset %d of the inflated stream: the name and the CIGAR do not fit" % off7)
    x = bytearray(b); struct.pack_into("<i", x, 4, 3); out["refid_beyond"] = (stream(7, bytes(x)), "offset %d of the inflated stream: a refID beyond" % off7)
    full = stream(40, b""); last = len(full) - len(rec_bytes(good[39]))
    out["cut_record"] = (full[:-5], "offset %d of the inflated stream: a record cut by the end" % last)
    out["cut_size_field"] = (full + b"\x40\0", "offset %d of the inflated stream: a record cut by the end" % len(full))
    out["cg_tag"] = (stream(7, rec_bytes(rec(0, 500, cig=[(100, "S"), (100, "N")], qname="cg"))), "holds a CIGAR of more than 65535 operations (CG tag): not supported")
    return out


def decode(path_or_bytes):
    """bam_util.read_bam's records as the dicts above (cig as text), the header text and the reference list"""
    import bam_util
    text, refs, recs, _ = bam_util.read_bam(path_or_bytes)
    return text, refs, recs


def as_read_bam(r):
    """a record dict above as bam_util.read_bam shows it"""
    tags = []
    t = r["tags"]
    while t:
        if t[2:3] == b"i":
            tags.append("%s:i:%d" % (t[:2].decode(), struct.unpack_from("<i", t, 3)[0])); t = t[7:]
        else:
            z = t.index(b"\0"); tags.append("%s:Z:%s" % (t[:2].decode(), t[3:z].decode())); t = t[z + 1:]
    n = r["l_seq"]
    return dict(qname=r["qname"], flag=r["flag"], rid=r["rid"], pos=r["pos"], mapq=r["mapq"], cigar="".join("%d%s" % c for c in r["cig"]) or "*", nrid=r["nrid"], npos=r["npos"], tlen=r["tlen"],
                seq="".join("AC"[i % 2] for i in range(n)) or "*", qual="?" * n if n else "*", tags=tags, bin=r["bin"])

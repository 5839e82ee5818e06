"""The rules of `airlift-align bam-index` (airlift_amd/csrc/al_dev_bai.h) restated in Python, independent of the C++: the interval and the bin of a record, the
virtual offsets from the table of BGZF members, the chunks, the linear index, pseudo-bin 37450 and n_no_coor (expected_bai); a parser of the BAI; and the query
procedure of the SAM specification, section 5.3 (query), which is what shows an index to be right: byte parity with samtools index is not claimed, since htslib's
order of the bins and its folding of bins into their parents are not part of the format.  And the directed inputs of the index's tests.

A case is (records, layout): records are the dicts of lift_cases.rec over the header HDR / REFS below, in coordinate order; layout says how the stream is cut into
BGZF members -- a block size, or ("cuts", offsets) for members that end exactly there, or ("empty", offset) for an empty member in the middle.  self_check() asserts
that the lists hold the shapes their comments claim, and that over a fixed list of regions the query through expected_bai finds exactly what a scan finds."""
import itertools
import struct

import lift_cases as lc
from select_cases import bgzf

MAX_END = 1 << 29
PSEUDO = 37450
PIECES = (1000, 4096)
BLOCKS = (700, 0xff00)
REFS = [("big", 1 << 29), ("s1", 100000), ("none_mid", 5000), ("s2", 70000), ("none_end", 3000)]
HDR = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS)
H0 = len(lc.header_bytes(HDR, REFS))
SHIFTS = (14, 17, 20, 23, 26)


class Refused(Exception):
    """the input has no BAI; the message holds what the command's message must contain"""


# ---- the rules -------------------------------------------------------------------------------------------------------------------------------------------------
def interval(r):
    """[beg, end) of a record with rid >= 0, and whether flag 4 is clear"""
    beg = max(r["pos"], 0); mapped = not r["flag"] & 4
    reflen = sum(l for l, o in r["cig"] if o in "MDN=X")
    return beg, beg + (reflen if mapped and reflen else 1), mapped


def members(data):
    """the BGZF members of a file: (file offset, stream offset, isize, msize)"""
    out, p, s = [], 0, 0
    while p < len(data):
        msize = struct.unpack_from("<H", data, p + 16)[0] + 1; isize = struct.unpack_from("<I", data, p + msize - 4)[0]
        out.append((p, s, isize, msize)); p += msize; s += isize
    assert p == len(data)
    return out


def voff(mem, s):
    """the virtual offset of stream offset s: the member that holds it (an empty one never does); behind the last byte: the file offset behind the last non-empty member"""
    for f, o, isize, msize in mem:
        if o <= s < o + isize:
            return f << 16 | (s - o)
    assert s == sum(m[2] for m in mem), s
    return max(f + msize for f, o, isize, msize in mem if isize) << 16


def key(r):
    return (1 << 64) - 1 if r["rid"] < 0 else r["rid"] << 32 | (r["pos"] & 0xffffffff)


def offsets(recs, h0=H0):
    out, p = [], h0
    for r in recs:
        out.append(p); p += len(lc.rec_bytes(r))
    return out, p


def expected_bai(refs, recs, mem, h0=H0):
    """the bytes of the index; Refused where the command refuses"""
    offs, end_s = offsets(recs, h0)
    rows = []                                                        # (rid, bin, beg, end, mapped, vbeg, vend) per placed record
    no_coor = 0
    for i, (r, s) in enumerate(zip(recs, offs)):
        if r["rid"] >= len(refs):
            raise Refused("malformed BAM record at offset %d of the inflated stream: a refID beyond" % s)
        beg, end, mapped = interval(r)
        if r["rid"] >= 0 and end > MAX_END:
            raise Refused("the record at offset %d of the inflated stream ends beyond 2^29" % s)
        if r["rid"] >= 0 and mapped and end > refs[r["rid"]][1]:
            raise Refused("the record at offset %d of the inflated stream ends beyond its contig's length" % s)
        if i and key(r) < key(recs[i - 1]):
            raise Refused("not in coordinate order at offset %d of the inflated stream" % s)
        if r["rid"] < 0:
            no_coor += 1; continue
        rows.append((r["rid"], lc.reg2bin(beg, end), beg, end, mapped, voff(mem, s), voff(mem, s + len(lc.rec_bytes(r)))))
    out = [b"BAI\1", struct.pack("<i", len(refs))]
    for rid in range(len(refs)):
        mine = [x for x in rows if x[0] == rid]
        bins = {}
        for (_, b), run in itertools.groupby(mine, key=lambda x: x[:2]):
            run = list(run); c = [run[0][5], run[-1][6]]
            if b in bins and bins[b][-1][1] >> 16 >= c[0] >> 16:
                bins[b][-1][1] = c[1]
            else:
                bins.setdefault(b, []).append(c)
        out.append(struct.pack("<i", len(bins) + (1 if mine else 0)))
        for b in sorted(bins):
            out.append(struct.pack("<Ii", b, len(bins[b])) + b"".join(struct.pack("<QQ", *c) for c in bins[b]))
        if mine:
            out.append(struct.pack("<IiQQQQ", PSEUDO, 2, mine[0][5], mine[-1][6], sum(1 for x in mine if x[4]), sum(1 for x in mine if not x[4])))
        lin = {}
        for x in mine:
            if x[4]:
                for w in range(x[2] >> 14, ((x[3] - 1) >> 14) + 1):
                    lin[w] = min(lin.get(w, x[5]), x[5])
        n_intv = max(lin) + 1 if lin else 0
        out.append(struct.pack("<i", n_intv))
        left, vals = 0, []
        for w in range(n_intv):
            left = lin.get(w, left); vals.append(left)
        out.append(struct.pack("<%dQ" % n_intv, *vals))
    out.append(struct.pack("<Q", no_coor))
    return b"".join(out)


def parse_bai(b):
    """-> (per contig dict(bins={bin: [(beg, end)]}, pseudo=(beg, end, mapped, unmapped) or None, ioffset=[...]), n_no_coor); the file must hold nothing else"""
    assert b[:4] == b"BAI\1"
    n_ref, = struct.unpack_from("<i", b, 4); p = 8; out = []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", b, p); p += 4; bins, pseudo, order = {}, None, []
        for _ in range(n_bin):
            bn, n_chunk = struct.unpack_from("<Ii", b, p); p += 8
            ch = [struct.unpack_from("<QQ", b, p + 16 * k) for k in range(n_chunk)]; p += 16 * n_chunk
            order.append(bn)
            if bn == PSEUDO:
                assert n_chunk == 2; pseudo = ch[0] + ch[1]
            else:
                assert bn < 37449 and bn not in bins and n_chunk >= 1; bins[bn] = ch
        assert order == sorted(order)
        n_intv, = struct.unpack_from("<i", b, p); p += 4
        io = list(struct.unpack_from("<%dQ" % n_intv, b, p)); p += 8 * n_intv
        out.append(dict(bins=bins, pseudo=pseudo, ioffset=io))
    no_coor, = struct.unpack_from("<Q", b, p); p += 8
    assert p == len(b)
    return out, no_coor


def reg2bins(beg, end):
    end -= 1; out = [0]
    for sh, off in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(off + (beg >> sh), off + (end >> sh) + 1)
    return out


def query(bai, bam, rid, beg, end):
    """The records of the BGZF file `bam` that overlap [beg, end) of contig rid, found through the index as the specification says: the chunks of reg2bins,
    without those that end at or before ioffset[beg >> 14]; the records of what is left, read from the file; those that overlap.  -> their stream offsets"""
    import gzip
    contigs, _ = parse_bai(bai)
    c = contigs[rid]
    io = c["ioffset"]; w = beg >> 14
    min_off = 0 if not io else io[w] if w < len(io) else io[-1]
    chunks = sorted(ch for b in reg2bins(beg, end) for ch in c["bins"].get(b, []) if ch[1] > min_off)
    mem = members(bam); stream = gzip.decompress(bam)
    at = {f: o for f, o, _, _ in mem}; at[len(bam)] = len(stream)
    for f, o, isize, msize in mem:
        at.setdefault(f + msize, o + isize)
    hits = set()
    for vb, ve in chunks:
        p, e = at[vb >> 16] + (vb & 0xffff), at[ve >> 16] + (ve & 0xffff)
        while p < e:
            bs, r_rid, pos, l_rn, _, _, n_cig, flag = struct.unpack_from("<iiiBBHHH", stream, p)
            cig = [(w_ >> 4, lc.CIG[w_ & 15]) for w_ in struct.unpack_from("<%dI" % n_cig, stream, p + 36 + l_rn)]
            b_, e_, _ = interval(dict(pos=pos, flag=flag, cig=cig))
            if r_rid == rid and b_ < end and e_ > beg:
                hits.add(p)
            p += 4 + bs
        assert p == e, (p, e)
    return sorted(hits)


def scan(recs, rid, beg, end, h0=H0):
    """the same answer by a scan of the records"""
    offs, _ = offsets(recs, h0)
    return [s for r, s in zip(recs, offs) if r["rid"] == rid and interval(r)[0] < end and interval(r)[1] > beg]


# ---- files and member tables -------------------------------------------------------------------------------------------------------------------------------------
def stream(recs):
    return lc.bam_bytes(HDR, REFS, recs)


def compress(blob, layout):
    if isinstance(layout, int):
        return bgzf(blob, layout)
    if layout[0] == "cuts":
        return lc.bgzf_at(blob, layout[1])
    assert layout[0] == "empty"
    return bgzf(blob[:layout[1]], 0xff00, eof=False) + bgzf(b"", 0xff00) + bgzf(blob[layout[1]:], 0xff00)


# ---- the directed inputs -----------------------------------------------------------------------------------------------------------------------------------------
def M(pos, n, name, rid=0, **kw):
    return lc.rec(rid, pos, qname=name, cig=((n, "M"),), **kw)


def U(name):
    return lc.rec(-1, -1, 4, cig=(), qname=name)


def boundary_points():
    return [3 << sh for sh in SHIFTS]


def boundaries():
    """records whose beg or end lies at -1, 0 and +1 of a multiple of 2^14, 2^17, 2^20, 2^23 and 2^26 (they move to the parent bin by one base), and a record that
    ends at exactly 2^29"""
    recs = []
    for m in boundary_points():
        for d in (-1, 0, 1):
            recs.append(M(m + d, 10, "b%d_%d" % (m, d)))                                  # beg at the boundary
            recs.append(M(m + d - 10, 10, "e%d_%d" % (m, d)))                             # end at the boundary
    recs.append(M(MAX_END - 50, 50, "last"))
    return sorted(recs, key=key)


def basics():
    """reflen 0 (CIGAR * and a CIGAR of I and S only), flag 4 with a position (behind its mapped mate, as a sorted BAM holds it), an N operation across five
    windows followed by records that start inside it, both small contigs, unplaced records at the tail"""
    recs = [M(100, 50, "a0"), lc.rec(0, 150, cig=(), qname="star"), lc.rec(0, 160, cig=((5, "I"), (7, "S")), qname="ins_clip"),
            M(20000, 30, "mate", flag=1 | 8 | 64), lc.rec(0, 20000, 4 | 1 | 128, cig=(), qname="mate", nrid=0, npos=20000),
            lc.rec(1, 1000, cig=((10, "M"), (5 << 14, "N"), (10, "M")), qname="long_n")]
    recs += [M(p, 10, "in%d" % p, rid=1) for p in (20000, 40000, 60000, 90000)]
    recs += [M(5, 10, "s2a", rid=3), M(69990, 10, "s2_end", rid=3)]
    recs += [U("u%d" % i) for i in range(3)]
    return recs


def counted(n):
    return [M(100 + 37 * i, 20, "c%d" % i, rid=1) for i in range(n)]


def bin_return():
    """bin 585, bin 4681, bin 585 again: the two runs of 585 are one chunk inside one member, two chunks across two members"""
    return [M(10, 20000, "wide0"), M(100, 10, "narrow"), M(200, 20000, "wide1"), M(300, 10, "after")]


def one_bin(n=300):
    """n records of one bin: a run that spans three pieces of 4096 bytes and more of 1000"""
    return [M(10 + i, 10, "o%03d" % i) for i in range(n)]


def cut_cases():
    """name -> (records, layout) with members cut at record boundaries"""
    out = {}
    recs = counted(20); offs, end = offsets(recs)
    out["ends_at_member_end"] = (recs, ("cuts", [offs[7]]))                       # record 6 ends exactly at a member's end, record 7 starts exactly at a member's start
    out["first_at_member_start"] = (recs, ("cuts", [H0]))
    big = counted(5) + [lc.sized_rec(300, rid=1, pos=400, qname="three")] + [M(500 + i, 10, "t%d" % i, rid=1) for i in range(5)]
    o2, _ = offsets(big)
    out["spans_three_members"] = (big, ("cuts", [o2[5] + 100, o2[5] + 200]))
    out["empty_member"] = (recs, ("empty", offs[9]))
    br = bin_return(); o3, _ = offsets(br)
    out["bin_return_two_members"] = (br, ("cuts", [o3[2]]))
    out["last_ends_file"] = (recs, ("cuts", [offs[19]]))
    return out


def block_cases():
    """name -> records, each compressed at every block size of BLOCKS and walked at every piece size"""
    out = {"boundaries": boundaries(), "basics": basics(), "header_only": [], "single": [M(77, 10, "one", rid=3)], "only_unplaced": [U("x"), U("y")],
           "bin_return_one_member": bin_return(), "one_bin": one_bin()}
    for n in (63, 64, 65, 200):
        out["n%d" % n] = counted(n)
    return out


def all_cases():
    """name -> (records, layout) over every block size and every cut"""
    out = {}
    for name, recs in block_cases().items():
        for b in BLOCKS:
            out["%s@%d" % (name, b)] = (recs, b)
    out.update(cut_cases())
    return out


def regions():
    """the fixed list of regions of self_check and of the tests: every boundary +-1, the whole contigs, a contig without a record, windows no record touches"""
    out = []
    for m in boundary_points():
        out += [(0, m - 1, m), (0, m, m + 1), (0, m + 1, m + 2), (0, m - 1, m + 1), (0, m - 11, m - 9), (0, m + 9, m + 11)]
    out += [(0, MAX_END - 1, MAX_END), (0, MAX_END - 51, MAX_END - 50), (0, 0, MAX_END), (1, 0, 100000), (2, 0, 5000), (3, 0, 70000), (4, 0, 3000),
            (0, 5 << 14, 6 << 14), (1, 95000, 100000), (1, 1005, 1006), (1, 30000, 30001), (1, 82939, 82940), (1, 82940, 82941), (0, 150, 151), (0, 160, 161), (0, 20000, 20001),
            (0, 0, 1), (0, 10, 11), (0, 20009, 20210), (3, 69999, 70000), (3, 15, 69990)]
    return out


def refusals():
    """name -> (records, what the message must say): descents inside a contig, of the refID, a placed record behind an unplaced one, a refID beyond the list,
    end > 2^29, end beyond the contig"""
    out = {}
    def case(name, recs):
        try:
            expected_bai(REFS, recs, members(bgzf(stream(recs), 0xff00)))
        except Refused as e:
            out[name] = (recs, str(e)); return
        raise AssertionError(name)
    good = counted(12)
    case("descent", good[:7] + [M(100, 20, "down", rid=1)] + good[7:])
    case("refid_descent", good[:7] + [M(5, 10, "back", rid=0)] + [M(900, 10, "z", rid=1)])
    case("placed_after_unplaced", good[:3] + [U("u"), M(5000, 10, "after", rid=1)])
    case("refid_beyond", good[:3] + [M(5, 10, "bad", rid=5)])
    case("beyond_2_29", [M(MAX_END - 49, 50, "big")])
    case("flag4_beyond_2_29", [lc.rec(0, MAX_END, 4, cig=(), qname="big4")])
    case("beyond_ln", good[:3] + [M(99995, 10, "over", rid=1)])
    return out


def boundary_descent(end):
    """records whose stream descends exactly where the first text ends at `end` (merge_cases.unsorted's `boundary`, over this header) -> (records, offset)"""
    import merge_cases as mc
    recs = [M(100 + 10 * i, 10, "b%03d" % i, rid=1) for i in range(3 * (end // 45 + 1))]
    n1, _ = mc.first_window(stream(recs), H0, end)
    recs[n1] = M(50, 10, "b%03d" % n1, rid=1)
    return recs, offsets(recs)[0][n1]


def self_check():
    cases = all_cases()
    b = boundaries()
    for sh in SHIFTS:
        m = 3 << sh
        assert {r["pos"] - m for r in b} >= {-1, 0, 1} and {interval(r)[1] - m for r in b} >= {-1, 0, 1}, sh
        level = lambda r: [i for i, s in enumerate((14, 17, 20, 23, 26, 29)) if interval(r)[0] >> s == (interval(r)[1] - 1) >> s][0]
        cross = [r for r in b if interval(r)[0] < m < interval(r)[1]]
        assert cross and all(SHIFTS[level(r) - 1] >= sh for r in cross) and any(SHIFTS[level(r) - 1] == sh for r in cross), sh       # one base over the boundary: the parent's bin
    assert any(interval(r)[1] == MAX_END for r in b)
    bs = basics()
    assert any(not r["cig"] and not r["flag"] & 4 and r["rid"] >= 0 for r in bs) and any(r["cig"] and all(o in "IS" for _, o in r["cig"]) for r in bs)
    assert any(r["flag"] & 4 and r["rid"] >= 0 for r in bs) and sum(1 for r in bs if r["rid"] < 0) == 3 and bs[-1]["rid"] < 0
    ln = [r for r in bs if r["qname"] == "long_n"][0]; lb, le, _ = interval(ln)
    assert (le - 1 >> 14) - (lb >> 14) >= 5 and sum(1 for r in bs if r["rid"] == 1 and lb < r["pos"] < le) >= 3
    assert {r["rid"] for r in bs if r["rid"] >= 0} == {0, 1, 3}                                         # contigs 2 and 4 get no record: one in the middle, one at the end
    bc = block_cases()
    assert bc["header_only"] == [] and len(bc["single"]) == 1 and [len(bc["n%d" % n]) for n in (63, 64, 65, 200)] == [63, 64, 65, 200]
    ob = one_bin(); assert len({lc.reg2bin(*interval(r)[:2]) for r in ob}) == 1 and offsets(ob)[1] - H0 > 3 * 4096
    br = [lc.reg2bin(*interval(r)[:2]) for r in bin_return()]; assert br[0] == br[2] != br[1]
    for name, (recs, layout) in sorted(cases.items()):
        assert all(key(x) <= key(y) for x, y in zip(recs, recs[1:])), name
        blob = stream(recs); data = compress(blob, layout); mem = members(data)
        import gzip
        assert gzip.decompress(data) == blob, name
        bai = expected_bai(REFS, recs, mem)
        contigs, no_coor = parse_bai(bai)
        assert no_coor == sum(1 for r in recs if r["rid"] < 0) and not contigs[2]["bins"] and not contigs[2]["ioffset"] and not contigs[4]["bins"] and contigs[4]["pseudo"] is None, name
        for rid, beg, end in regions():
            assert query(bai, data, rid, beg, end) == scan(recs, rid, beg, end), (name, rid, beg, end)
    cc = cut_cases()
    recs, layout = cc["ends_at_member_end"]; mem = members(compress(stream(recs), layout)); offs, _ = offsets(recs)
    assert any(o == offs[7] and i for _, o, i, _ in mem) and voff(mem, offs[7]) & 0xffff == 0                 # the end of record 6 is (next member, 0)
    recs, layout = cc["spans_three_members"]; mem = members(compress(stream(recs), layout)); offs, _ = offsets(recs)
    assert len({voff(mem, s) >> 16 for s in (offs[5], offs[5] + 150, offs[5] + 299)}) == 3
    recs, layout = cc["empty_member"]; mem = members(compress(stream(recs), layout))
    assert any(i == 0 for _, _, i, _ in mem[:-1]) and voff(mem, offsets(recs)[0][9]) >> 16 > [f for f, _, i, _ in mem if i == 0][0]
    one = parse_bai(expected_bai(REFS, bin_return(), members(compress(stream(bin_return()), 0xff00))))[0][0]["bins"]
    recs, layout = cc["bin_return_two_members"]
    two = parse_bai(expected_bai(REFS, recs, members(compress(stream(recs), layout))))[0][0]["bins"]
    assert len(one[585]) == 1 and len(two[585]) == 2
    long_io = parse_bai(expected_bai(REFS, bs, members(compress(stream(bs), 0xff00))))[0][1]["ioffset"]
    assert len(set(long_io[0:6])) == 1 and long_io[0] != 0                                            # the later windows' ioffset stays the long record's
    assert sorted(refusals()) == ["beyond_2_29", "beyond_ln", "descent", "flag4_beyond_2_29", "placed_after_unplaced", "refid_beyond", "refid_descent"]
    return cases


# ---- the taps ----------------------------------------------------------------------------------------------------------------------------------------------------
def tap(L, blob, mem, file_end, piece, dev=None, expect=0):
    """an uncompressed stream and its member table through the piece loop of the host twin (dev None) or of the kernels -> the index's bytes"""
    import ctypes as C
    n = len(mem)
    mf = (C.c_uint64 * n)(*[m[0] for m in mem]); ms = (C.c_uint64 * n)(*[m[1] for m in mem]); mi = (C.c_uint32 * n)(*[m[2] for m in mem])
    cap = 1 << 20; out = C.create_string_buffer(cap); got, held = C.c_size_t(0), C.c_size_t(0)
    if dev is None:
        rc = L.al_dbg_bai_host(blob, len(blob), mf, ms, mi, n, file_end, piece, out, cap, C.byref(got))
    else:
        rc = L.al_dbg_bai(dev, blob, len(blob), mf, ms, mi, n, file_end, piece, out, cap, C.byref(got), C.byref(held))
    assert rc == expect, rc
    assert held.value == 0
    return out.raw[:got.value]


# ---- the shapes tests/csrc/index_main.cpp generates (the same tables stand there) ----------------------------------------------------------------------------------
SAN_MEMBER = 333            # stream bytes per member of the synthetic table; member k lies at file offset 1000 k and is 1000 bytes long


def san_specs():
    """name -> segments (rid, pos0, step, count, reflen, name prefix); rid -1: unplaced records.  Names that begin with `refused` do not index."""
    return {"one_bin": [(0, 10, 1, 300, 10, "o")],
            "bins": [(0, 10, 4000, 40, 20000, "w"), (0, 200000, 16384, 30, 10, "n"), (1, 5, 7, 100, 30, "s")],
            "contigs": [(0, 100, 50, 20, 10, "a"), (1, 100, 50, 20, 10, "b"), (3, 100, 50, 20, 10, "c"), (-1, -1, 0, 5, 0, "u")],
            "top": [(0, (1 << 29) - 1000, 10, 90, 100, "t")],
            "header_only": [],
            "refused_descent": [(1, 100, 10, 30, 10, "a"), (1, 90, 1, 1, 10, "down"), (1, 500, 10, 30, 10, "b")],
            "refused_after_unplaced": [(1, 100, 10, 3, 10, "a"), (-1, -1, 0, 1, 0, "u"), (1, 900, 1, 1, 10, "z")],
            "refused_big": [(0, (1 << 29) - 5, 1, 1, 10, "big")],
            "refused_ln": [(3, 69995, 1, 1, 10, "over")]}


def from_spec(segs):
    return [U(pre + str(i)) if rid < 0 else M(pos0 + i * step, reflen, pre + str(i), rid=rid) for rid, pos0, step, count, reflen, pre in segs for i in range(count)]


def san_members(n_stream):
    k = (n_stream + SAN_MEMBER - 1) // SAN_MEMBER
    return [(1000 * i, SAN_MEMBER * i, min(SAN_MEMBER, n_stream - SAN_MEMBER * i), 1000) for i in range(k)], 1000 * k


def fnv(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h

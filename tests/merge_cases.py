"""The rules of `airlift-align merge` (airlift_amd/csrc/al_dev_merge.h) restated in Python, independent of the C++: the key, the order with its tie rule, the
merged reference list with the refID translation, the merged header text.  And the directed inputs of the merge's tests: runs sized around the tile of
k_merge_tile, ties, windows that end inside runs of equal keys, reference lists that differ, header lines that collide, unsorted and malformed inputs.

An input is (header text, reference list, records); records are the dicts of lift_cases.rec.  self_check() asserts that the lists have the properties their
comments claim -- that the straddling runs really straddle for the tile and the piece sizes used -- so that a change of either cannot silently defuse a case."""
import struct

import lift_cases as lc

NOKEY = (1 << 64) - 1
PIECES = (1000, 4096)
HDR = lc.HEADER
REFS = lc.REFS


class Refused(Exception):
    """the inputs' headers do not merge; the message holds what the command's message must contain"""


# ---- the rules -------------------------------------------------------------------------------------------------------------------------------------------------
def key(r):
    return NOKEY if r["rid"] < 0 else r["rid"] << 32 | (r["pos"] & 0xffffffff)


def merged_refs(inputs):
    """-> (the output's reference list, per input the table old refID -> new refID)"""
    refs, maps = list(inputs[0][1]), [list(range(len(inputs[0][1])))]
    for text, rl, _ in inputs[1:]:
        m = []
        for name, ln in rl:
            names = [x[0] for x in refs]
            if name in names:
                j = names.index(name)
                if refs[j][1] != ln:
                    raise Refused("contig '%s' has length %d here and %d in" % (name, ln, refs[j][1]))
            else:
                j = len(refs); refs.append((name, ln))
            if m and j <= m[-1]:
                raise Refused("contigs '%s' and '%s' stand in the other order" % (rl[len(m) - 1][0], name))
            m.append(j)
        maps.append(m)
    return refs, maps


def _is(l, t):
    return l[:3] == t and (len(l) == 3 or l[3] == "\t")


def _field(l, pre):
    for f in l.split("\t")[1:]:
        if f.startswith(pre):
            return f[len(pre):]
    return None


def merged_header(inputs):
    """the header text of the merged BAM"""
    refs, _ = merged_refs(inputs)
    n_before = len(inputs[0][1])
    lines = inputs[0][0].split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    out = [] if any(_is(l, "@HD") for l in lines) else ["@HD\tVN:1.6\tSO:coordinate"]
    for l in lines:
        if _is(l, "@HD"):
            f = ["SO:coordinate" if x[:3] == "SO:" else x for x in l.split("\t")]
            l = "\t".join(f if "SO:coordinate" in f else f + ["SO:coordinate"])
        out.append(l)
    known = [x[0] for x in inputs[0][1]]
    for k, (text, rl, _) in enumerate(inputs[1:], start=2):
        own = [l for l in text.split("\n") if l]
        for name, ln in rl:
            if name not in known:
                known.append(name)
                sq = [l for l in own if _is(l, "@SQ") and _field(l, "SN:") == name]
                out.append(sq[0] if sq else "@SQ\tSN:%s\tLN:%d" % (name, ln))
        for l in own:
            if _is(l, "@HD") or _is(l, "@SQ"):
                continue
            if _is(l, "@CO"):
                out.append(l); continue
            if l in out:
                continue
            for t in ("@PG", "@RG"):
                if _is(l, t) and _field(l, "ID:") is not None and any(_is(o, t) and _field(o, "ID:") == _field(l, "ID:") for o in out):
                    if t == "@RG":
                        raise Refused("the @RG line with ID '%s' differs" % _field(l, "ID:"))
                    i = _field(l, "ID:")
                    l = l.replace("\tID:" + i, "\tID:%s.%d" % (i, k), 1)
            out.append(l)
    assert len(known) == len(refs) and n_before <= len(refs)
    return "".join(x + "\n" for x in out)


def expected(inputs):
    """the merged records: (input, index in input, the record with its refIDs translated), sorted by (key, input, index)"""
    _, maps = merged_refs(inputs)
    out = []
    for i, (_, rl, recs) in enumerate(inputs):
        for x, r in enumerate(recs):
            o = dict(r)
            for f in ("rid", "nrid"):
                if r[f] >= 0:
                    assert r[f] < len(rl)
                    o[f] = maps[i][r[f]]
            out.append((key(o), i, x, o))
    out.sort(key=lambda t: t[:3])
    return [(i, x, o) for _, i, x, o in out]


def expected_stream(inputs):
    """the inflated bytes of the merged BAM"""
    return lc.header_bytes(merged_header(inputs), merged_refs(inputs)[0]) + b"".join(lc.rec_bytes(o) for _, _, o in expected(inputs))


def stream(inp):
    return lc.bam_bytes(inp[0], inp[1], inp[2])


def descends(recs):
    return any(key(b) < key(a) for a, b in zip(recs, recs[1:]))


# ---- the directed inputs -----------------------------------------------------------------------------------------------------------------------------------------
def R(pos, name, rid=0, **kw):
    return lc.rec(rid, pos, qname=name, cig=((10, "M"),), **kw)


def U(name):
    return lc.rec(-1, -1, 4, cig=(), qname=name)


def inp(recs, text=HDR, refs=REFS):
    return (text, list(refs), list(recs))


def tiles(T):
    """name -> [A, B]: run sizes around the tile, keys strictly interleaved, all of A below all of B, and the reverse"""
    out = {}
    for na, nb in ((0, 1), (1, 0), (1, 1), (T - 1, 1), (T, T), (T + 1, T - 1), (2 * T + 1, 3), (3, 2 * T + 1)):
        m = max(na, nb)
        out["inter_%d_%d" % (na, nb)] = [inp(R(10 + 2 * i * m // max(na, 1), "a%d" % i) for i in range(na)), inp(R(11 + 2 * i * m // max(nb, 1), "b%d" % i) for i in range(nb))]
        out["a_below_%d_%d" % (na, nb)] = [inp(R(10 + i, "a%d" % i) for i in range(na)), inp(R(10 + na + i, "b%d" % i) for i in range(nb))]
        out["b_below_%d_%d" % (na, nb)] = [inp(R(10 + nb + i, "a%d" % i) for i in range(na)), inp(R(10 + i, "b%d" % i) for i in range(nb))]
    return out


def ties(T):
    out = {}
    out["all_equal"] = [inp(R(100, "a%d" % i) for i in range(T + 1)), inp(R(100, "b%d" % i) for i in range(T + 1))]
    # 5 + 2T + 1 and 3 + 2T + 2 records: the 4T equal keys of the result begin at index 8 and cross every tile boundary up to 4T
    out["straddle"] = [inp([R(10 + i, "al%d" % i) for i in range(5)] + [R(500, "a%d" % i) for i in range(2 * T)] + [R(900, "ah")]),
                       inp([R(20 + i, "bl%d" % i) for i in range(3)] + [R(500, "b%d" % i) for i in range(2 * T)] + [R(901, "bh0"), R(902, "bh1")])]
    out["unmapped_both"] = [inp([R(10 + 3 * i, "a%d" % i, rid=i // 20) for i in range(40)] + [U("au%d" % i) for i in range(3)]),
                            inp([R(11 + 3 * i, "b%d" % i, rid=i // 20) for i in range(40)] + [U("bu%d" % i) for i in range(4)])]
    out["unmapped_one"] = [inp([R(10 + 3 * i, "a%d" % i) for i in range(40)]), inp([R(11 + 3 * i, "b%d" % i) for i in range(40)] + [U("bu%d" % i) for i in range(4)])]
    out["equal_diff_len"] = [inp([R(100, "x"), R(100, "a_much_longer_name_y", tags=lc.NM), R(200, "p")]), inp([R(100, "zz", l_seq=7), R(100, "w"), R(200, "a_long_name_q"), R(200, "r")])]
    return out


def _n(piece):
    return piece // 45 + 1          # (records of 45 to 49 bytes: about one piece's worth)


def windows(piece):
    """name -> inputs for the round loop with windows of `piece` bytes"""
    n = _n(piece); out = {}
    run = lambda c, k, pos: [R(pos, "%se%d" % (c, i)) for i in range(k)]
    low = lambda c, k, p0: [R(p0 + i, "%sl%d" % (c, i)) for i in range(k)]
    high = lambda c, k, p0: [R(p0 + i, "%sh%d" % (c, i)) for i in range(k)]
    # A's run of key 5000 crosses A's first window's end while B holds 5000 inside its first window: B's must wait for the rest of A's
    out["cross_a"] = [inp(low("a", n // 2, 100) + run("a", n, 5000) + high("a", n, 6000)), inp(low("b", 3, 50) + run("b", 3, 5000) + high("b", 2 * n, 5500))]
    # the roles swapped: B's run crosses B's window's end, A (an earlier input than j*) holds the key inside its window and emits it at once
    out["cross_b"] = [inp(low("a", 3, 50) + run("a", 3, 5000) + high("a", 2 * n, 5500)), inp(low("b", n // 2, 100) + run("b", n, 5000) + high("b", n, 6000))]
    out["dense"] = [inp(R(10 + i, "a%d" % i) for i in range(8 * n)), inp(R(10 + 2 * n * i, "b%d" % i) for i in range(5))]
    big = lc.sized_rec(2 * piece + 101, pos=300, qname="big")
    out["big_record"] = [inp(low("a", 5, 100) + [big] + high("a", n, 400)), inp(low("b", n, 90) + high("b", n, 350))]
    out["header_only"] = [inp(low("a", 2 * n, 100)), inp([])]
    out["header_only_first"] = [inp([]), inp(low("b", 2 * n, 100))]
    for k in (3, 8):
        out["k%d" % k] = [inp(low(chr(97 + i), n // 2 + i, 100 + i) + run(chr(97 + i), n // 3 + 2 * i + 1, 5000) + high(chr(97 + i), n // 2, 6000 + i)) for i in range(k)]
    out["early_eof"] = [inp(low("a", 3, 10)), inp(low("b", 3 * n, 5)), inp(low("c", 2, 7))]
    return out


def refs_cases():
    """name -> inputs whose reference lists differ"""
    sub = [("chrB", 8000), ("chrC", 5000)]
    a = [R(100 + 10 * i, "a%d" % i, rid=i // 10) for i in range(30)]
    b = [R(105, "p0", rid=0, flag=1 | 64, nrid=1, npos=300, tlen=0), R(205, "p1", rid=0, flag=1 | 8 | 64), R(300, "p0", rid=1, flag=1 | 128, nrid=0, npos=105), R(400, "s", rid=1), U("bu")]
    new = [("chrA", 10000), ("chrC", 5000), ("chrD", 500)]
    c = [R(7, "c0", rid=0), R(8, "c1", rid=1, flag=1 | 64, nrid=2, npos=9), R(9, "c2", rid=2, flag=1 | 128, nrid=1, npos=8), R(10, "c3", rid=2)]
    hdr_new = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chrA\tLN:10000\n@SQ\tSN:chrC\tLN:5000\n@SQ\tSN:chrD\tLN:500\tM5:abc\n"
    return {"subset": [inp(a), inp(b, refs=sub)], "new_contig": [inp(a), inp(c, text=hdr_new, refs=new)], "new_contig_no_sq": [inp(a), inp(c, text="@CO\tno SQ lines\n", refs=new)],
            "three": [inp(a), inp(b, refs=sub), inp(c, text=hdr_new, refs=new)]}


def refs_refusals():
    """name -> (inputs, what the message must say)"""
    a = [R(100 + 10 * i, "a%d" % i, rid=i // 10) for i in range(30)]
    beyond = [R(5, "ok"), R(6, "bad", rid=3), R(7, "ok2")]
    off = len(lc.header_bytes(HDR, REFS)) + len(lc.rec_bytes(beyond[0]))
    return {"ln_mismatch": ([inp(a), inp([R(5, "b")], refs=[("chrA", 9999)])], "contig 'chrA' has length 9999 here and 10000 in"),
            "non_monotone": ([inp(a), inp([R(5, "b")], refs=[("chrB", 8000), ("chrA", 10000)])], "contigs 'chrB' and 'chrA' stand in the other order"),
            "refid_beyond": ([inp(a), inp(beyond)], "offset %d of the inflated stream: a refID beyond" % off),
            "next_refid_beyond": ([inp(a), inp([R(5, "ok"), R(6, "bad", flag=1, nrid=9, npos=1), R(7, "ok2")])], "offset %d of the inflated stream: a refID beyond" % off)}


SQ = "@SQ\tSN:chrA\tLN:10000\n@SQ\tSN:chrB\tLN:8000\n@SQ\tSN:chrC\tLN:5000\n"


def headers():
    """name -> inputs (two records each) whose header lines meet every rule of the text"""
    a, b = [R(10, "a")], [R(5, "b")]
    hd = "@HD\tVN:1.6\tSO:coordinate\n"
    two = lambda t1, t2: [inp(a, text=t1), inp(b, text=t2)]
    return {"pg_dedup": two(hd + SQ + "@PG\tID:x\tPN:x\n", hd + SQ + "@PG\tID:x\tPN:x\n@PG\tID:y\tPN:y\tPP:x\n"),
            "pg_collide": two(hd + SQ + "@PG\tID:x\tPN:x\n", hd + SQ + "@PG\tID:x\tPN:other\tPP:w\n@PG\tID:xx\tPN:x\n"),
            "rg_same": two(hd + SQ + "@RG\tID:g\tSM:s\n", hd + SQ + "@RG\tID:g\tSM:s\n@RG\tID:h\tSM:s\n"),
            "co": two(hd + SQ + "@CO\thello\n", hd + SQ + "@CO\thello\n@CO\tworld\n"),
            "no_hd": two(SQ + "@PG\tID:x\n", hd + SQ),
            "so_unsorted": two("@HD\tVN:1.6\tSO:unsorted\tGO:none\n" + SQ, "@HD\tVN:1.5\tSO:coordinate\n" + SQ),
            "hd_no_so": two("@HD\tVN:1.6\n" + SQ, ""),
            "empty": two("", "")}


def header_refusals():
    hd = "@HD\tVN:1.6\tSO:coordinate\n"
    return {"rg_collide": ([inp([R(10, "a")], text=hd + SQ + "@RG\tID:g\tSM:a\n"), inp([R(5, "b")], text=hd + SQ + "@RG\tID:g\tSM:b\n")], "the @RG line with ID 'g' differs")}


def first_window(blob, start, end):
    """the complete records of blob[start:end): how many, and the offset behind the last"""
    p, n = start, 0
    while p + 4 <= end:
        bs = struct.unpack_from("<i", blob, p)[0]
        if p + 4 + bs > end:
            break
        p += 4 + bs; n += 1
    return n, p


H0 = len(lc.header_bytes(HDR, REFS))
# where the first text of a stream ends: the taps cut the stream behind the header into pieces; the command takes whole BGZF members until the piece is covered
ENDS = {("tap", 1000): H0 + 1000, ("tap", 4096): H0 + 4096, ("cli700", 1000): 1400, ("cli700", 4096): 4200}


def unsorted(end=None):
    """name -> (inputs, the index in input 2 of the record that is below the one before it).  end: where input 2's first text ends (ENDS), for the descent
    that lies exactly at a window's end: the last record of one window against the first of the next"""
    good = [R(100 + 10 * i, "a%d" % i) for i in range(60)]
    out = {}
    mid = [R(100 + 10 * i, "b%d" % i) for i in range(12)]; mid[7] = R(100, "down")
    out["mid"] = ([inp(good), inp(mid)], 7)
    um = [R(100, "b0"), U("u"), R(200, "after_unmapped")]
    out["mapped_after_unmapped"] = ([inp(good), inp(um)], 2)
    if end is not None:
        recs = [R(100 + 10 * i, "b%03d" % i) for i in range(3 * _n(end))]
        n1, _ = first_window(lc.bam_bytes(HDR, REFS, recs), H0, end)
        recs[n1] = R(50, "b%03d" % n1)                                # (the same length: the windows stay where they are)
        out["boundary"] = ([inp(good), inp(recs)], n1)
    return out


def unsorted_offset(inputs, idx):
    return H0 + sum(len(lc.rec_bytes(r)) for r in inputs[1][2][:idx])


def malformed():
    """name -> (input 1, the uncompressed stream of input 2, what the message must say): the shapes of lift_cases.malformed() that the walk judges, among
    records that are in order"""
    good = [R(100 + 10 * i, "g%d" % i) for i in range(40)]; h = lc.header_bytes(HDR, REFS); out = {}
    def at(k, bad):
        return h + b"".join(lc.rec_bytes(r) for r in good[:k]) + bad + b"".join(lc.rec_bytes(r) for r in good[k:])
    b = lc.rec_bytes(good[7]); off7 = len(h) + sum(len(lc.rec_bytes(r)) for r in good[:7])
    out["size31"] = (at(7, struct.pack("<i", 31) + b"\0" * 31), "offset %d of the inflated stream: block_size below 32" % off7)
    out["size_big"] = (at(7, struct.pack("<i", (1 << 28) + 1) + b[4:]), "offset %d of the inflated stream: block_size below 32" % off7)
    out["size_negative"] = (at(7, struct.pack("<i", -5) + b[4:]), "offset %d of the inflated stream: block_size below 32" % off7)
    full = at(40, b""); last = len(full) - len(lc.rec_bytes(good[39]))
    out["cut_record"] = (full[:-5], "offset %d of the inflated stream: a record cut by the end" % last)
    out["cut_size_field"] = (full + b"\x40\0", "offset %d of the inflated stream: a record cut by the end" % len(full))
    first = inp([R(100 + 7 * i, "a%d" % i) for i in range(30)])
    return {k: (first, v[0], v[1]) for k, v in out.items()}


def cli_pair(W):
    """the command's matrix input: lc.directed(257) split by parity of index plus the `long` and `cut1` walk sets, each half put in coordinate order (the merge
    takes sorted inputs; a stable sort keeps the records' relative order)"""
    recs = lc.directed(257); ws = lc.walk_sets(W)
    a = sorted(recs[0::2] + ws["long"], key=key); b = sorted(recs[1::2] + ws["cut1"], key=key)
    return [inp(a), inp(b)]


def self_check(T):
    """asserts the properties above; returns {list name: {case name: inputs}} of the sets that merge"""
    all_ = {"tiles": tiles(T), "ties": ties(T), "refs": refs_cases(), "headers": headers()}
    for p in PIECES:
        all_["windows%d" % p] = windows(p)
    for lname, cases in all_.items():
        for name, ins in cases.items():
            assert 2 <= len(ins) <= 8, (lname, name)
            for i in ins:
                assert not descends(i[2]), (lname, name)
            expected_stream(ins)
    t = tiles(T)
    assert [len(i[2]) for i in t["inter_%d_%d" % (T + 1, T - 1)]] == [T + 1, T - 1]
    for na, nb in ((T, T), (2 * T + 1, 3), (3, 2 * T + 1)):
        e = [i for i, _, _ in expected(t["inter_%d_%d" % (na, nb)])]
        assert sum(1 for x, y in zip(e, e[1:]) if x != y) >= 2 * min(na, nb) - 1                    # strictly interleaved
        e = [i for i, _, _ in expected(t["b_below_%d_%d" % (na, nb)])]
        assert e == [1] * nb + [0] * na
    e = expected(ties(T)["straddle"]); ks = [key(o) for _, _, o in e]
    lo, hi = ks.index(500), len(ks) - 1 - ks[::-1].index(500)
    assert hi - lo + 1 == 4 * T and lo // T != hi // T and lo % T != 0                                   # the equal run crosses tile boundaries and starts inside a tile
    assert [i for i, _, _ in e[lo:hi + 1]] == [0] * (2 * T) + [1] * (2 * T)
    e = expected(ties(T)["all_equal"]); assert [i for i, _, _ in e] == [0] * (T + 1) + [1] * (T + 1)
    for p in PIECES:
        w = windows(p)
        for name, who in (("cross_a", 0), ("cross_b", 1)):
            ins = w[name]; s = stream(ins[who]); n1, _ = first_window(s, H0, H0 + p)
            ks = [key(r) for r in ins[who][2]]; E = 5000
            assert ks[n1 - 1] == E and ks[n1] == E, (p, name)                                          # the run crosses the first window's end
            other = ins[1 - who]; m1, _ = first_window(stream(other), H0, H0 + p); ko = [key(r) for r in other[2]]
            assert E in ko[:m1] and ko[m1 - 1] > E, (p, name)                                          # the other input holds the key inside its first window
        assert len(stream(w["dense"][0])) > 6 * p and len(stream(w["dense"][1])) < p + H0
        assert any(len(lc.rec_bytes(r)) > 2 * p for r in w["big_record"][0][2])
        for k in (3, 8):
            assert len(w["k%d" % k]) == k and all(5000 in [key(r) for r in i[2]] for i in w["k%d" % k])
        for who in ("tap", "cli700"):
            ins, idx = unsorted(ENDS[who, p])["boundary"]
            n1, _ = first_window(stream(ins[1]), H0, ENDS[who, p])
            assert idx == n1 and key(ins[1][2][idx]) < key(ins[1][2][idx - 1]) and not descends(ins[1][2][:idx]) and not descends(ins[1][2][idx:])
    for name, (ins, idx) in unsorted().items():
        assert key(ins[1][2][idx]) < key(ins[1][2][idx - 1]) and not descends(ins[0][2])
    ins, idx = unsorted()["mapped_after_unmapped"]; assert key(ins[1][2][idx - 1]) == NOKEY
    for name, (ins, say) in list(refs_refusals().items())[:2] + list(header_refusals().items()):
        try:
            merged_header(ins); raise AssertionError(name)
        except Refused as e:
            assert str(e) in say or say in str(e), (name, str(e), say)
    return all_


# ---- the shapes tests/csrc/merge_main.cpp generates (the same tables stand there) ---------------------------------------------------------------------------------
def san_specs(T):
    """name -> per input a list of segments (rid, pos0, step, count, name prefix); rid -1: unmapped records.  Record i of a segment lies at pos0 + i * step and is
    named prefix + str(i).  The windows shapes at both piece sizes, the ties shapes, and the unsorted ones (their names begin with `unsorted`)"""
    out = {}
    for p in PIECES:
        n = _n(p); w = {}
        w["cross_a"] = [[(0, 100, 1, n // 2, "al"), (0, 5000, 0, n, "ae"), (0, 6000, 1, n, "ah")], [(0, 50, 1, 3, "bl"), (0, 5000, 0, 3, "be"), (0, 5500, 1, 2 * n, "bh")]]
        w["cross_b"] = w["cross_a"][::-1]
        w["dense"] = [[(0, 10, 1, 8 * n, "a")], [(0, 10, 2 * n, 5, "b")]]
        w["header_only"] = [[(0, 100, 1, 2 * n, "al")], []]
        for k in (3, 8):
            w["k%d" % k] = [[(0, 100 + i, 1, n // 2 + i, chr(97 + i) + "l"), (0, 5000, 0, n // 3 + 2 * i + 1, chr(97 + i) + "e"), (0, 6000 + i, 1, n // 2, chr(97 + i) + "h")] for i in range(k)]
        w["early_eof"] = [[(0, 10, 1, 3, "al")], [(0, 5, 1, 3 * n, "bl")], [(0, 7, 1, 2, "cl")]]
        for name, v in w.items():
            out["w%d_%s" % (p, name)] = v
    out["all_equal"] = [[(0, 100, 0, T + 1, "a")], [(0, 100, 0, T + 1, "b")]]
    out["straddle"] = [[(0, 10, 1, 5, "al"), (0, 500, 0, 2 * T, "a"), (0, 900, 1, 1, "ah")], [(0, 20, 1, 3, "bl"), (0, 500, 0, 2 * T, "b"), (0, 901, 1, 2, "bh")]]
    out["unmapped_both"] = [[(0, 10, 3, 20, "a"), (1, 10, 3, 20, "aa"), (-1, -1, 0, 3, "au")], [(0, 11, 3, 20, "b"), (1, 11, 3, 20, "bb"), (-1, -1, 0, 4, "bu")]]
    out["unsorted_mid"] = [[(0, 100, 10, 60, "a")], [(0, 100, 10, 7, "b"), (0, 100, 0, 1, "down"), (0, 180, 10, 40, "c")]]
    out["unsorted_after_unmapped"] = [[(0, 100, 10, 60, "a")], [(0, 100, 1, 1, "b"), (-1, -1, 0, 1, "u"), (0, 200, 1, 1, "after")]]
    out["unsorted_first"] = [[(0, 100, 10, 30, "a"), (0, 90, 1, 1, "down")], [(0, 5, 1, 50, "b")]]
    return out


def from_spec(spec):
    return [inp([U(pre + str(i)) if rid < 0 else R(pos0 + i * step, pre + str(i), rid=rid) for rid, pos0, step, count, pre in segs for i in range(count)]) for segs in spec]


def fnv(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return h

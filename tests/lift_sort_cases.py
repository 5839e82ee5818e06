"""The order of `airlift-align lift --sorted` (ORDER in airlift_amd/csrc/al_dev_lift.h) restated in Python -- the rules of lift_cases.py, then Python's stable
`sorted` on the key -- and the directed inputs that aim at the edges of the compaction, the descent count, the sort and the permuted gather: kept counts around
the wavefront and block sizes, pieces in order, pieces with exactly one descent, equal keys, keys that differ in one half only, records without a position,
positions near 2^31, and records of very different lengths.  lift_cases.py is imported, not changed."""
import gzip
import struct

import lift_cases as lc

NONE = (1 << 64) - 1


def key(k):
    """the sort key of a kept record (a dict of lift_cases.py), after the lift"""
    return NONE if k["rid"] < 0 else k["rid"] << 32 | (k["pos"] & 0xffffffff)


def truth(chain_text, refs, recs):
    """-> dict: verdicts, kept (sorted, dicts), perm (record index of every packed record), descents, packed bytes, rows, keys (sorted)"""
    v, kept, rows = lc.lift_all(chain_text, refs, recs)
    idx = [i for i, a in enumerate(v) if a != lc.UNLIFTED]
    keys = [key(k) for k in kept]
    order = sorted(range(len(kept)), key=lambda j: keys[j])                # (stable)
    return dict(v=v, kept=[kept[j] for j in order], perm=[idx[j] for j in order], descents=sum(1 for a, b in zip(keys, keys[1:]) if b < a),
                packed=b"".join(lc.rec_bytes(kept[j]) for j in order), rows=rows, keys=[keys[j] for j in order], unsorted=b"".join(lc.rec_bytes(k) for k in kept))


def sorted_header(text, tab):
    """the header text of the sorted lifted BAM: lift_cases.lift_header, the @HD line saying SO:coordinate (made, as the first line, where there is none)"""
    lines = lc.lift_header(text, tab).split("\n")[:-1]
    is_hd = lambda l: l[:3] == "@HD" and (len(l) == 3 or l[3] == "\t")
    if not any(is_hd(l) for l in lines):
        lines.insert(0, "@HD\tVN:1.6\tSO:coordinate")
    out = []
    for l in lines:
        if is_hd(l):
            f = ["SO:coordinate" if x[:3] == "SO:" else x for x in l.split("\t")]
            l = "\t".join(f if "SO:coordinate" in f else f + ["SO:coordinate"])
        out.append(l)
    return "".join(x + "\n" for x in out)


def inflate(path):
    """the inflated stream of a BGZF file"""
    return gzip.decompress(open(path, "rb").read())


def split_records(stream):
    """the record bytes of an uncompressed BAM stream, behind its header"""
    l_text = struct.unpack_from("<i", stream, 4)[0]; p = 8 + l_text
    n_ref = struct.unpack_from("<i", stream, p)[0]; p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", stream, p)[0]
    out = []
    while p < len(stream):
        n = 4 + struct.unpack_from("<i", stream, p)[0]; out.append(stream[p:p + n]); p += n
    return out


# ---- the directed inputs (behind lc.HEADER / lc.REFS, through lc.CHAIN unless a set names its own) ------------------------------------------------------------------
# chrA [2150, 4000) lifts to newA (refID 0) with d = 250, chrA [100, 1100) with d = 200, chrB [4000, 6000) to newB (refID 1) with d = -3000; chrC is not in the chain
def K(pos, name, rid=0, cig=((10, "M"),), **kw):
    return lc.rec(rid, pos, cig=cig, qname=name, **kw)


def U(name):
    return lc.rec(2, 500, qname=name)                   # unlifted: a contig the chain lacks


def N(name):
    return lc.rec(-1, -1, 4, cig=(), qname=name)        # kept, without a position: key ~0


def interleave(kept):
    """unlifted records in front and behind every second kept record, so that a kept record's compacted index is not its record index"""
    out = [U("u_first")]
    for i, r in enumerate(kept):
        out.append(r)
        if i % 2 == 1 or i % 7 == 0:
            out.append(U("u%d" % i))
    return out


def scattered(n, seed=12345):
    """n kept records at pseudo-random places of three blocks on two new contigs, a few without a position: out of order, with ties"""
    out, x = [], seed
    for i in range(n):
        x = (x * 1103515245 + 12345) & 0x7fffffff
        w = x >> 8
        if w % 11 == 0:
            out.append(N("n%d" % i))
        elif w % 3 == 0:
            out.append(K(4000 + (w >> 4) % 1900, "b%d" % i, rid=1))
        elif w % 3 == 1:
            out.append(K(2150 + (w >> 4) % 1800, "a%d" % i))
        else:
            out.append(K(100 + (w >> 4) % 64, "t%d" % i))                   # (few distinct positions: equal keys)
    return out


KEPT_EDGES = (0, 1, 2, 63, 64, 65, 255, 256, 257)
ONE_DESCENT_N = 300
ONE_DESCENT_AT = (1, 64, 256, ONE_DESCENT_N - 1)

BIG_CHAIN = """chain 1000 chrA 10000 + 100 500 big 2147483647 + 2147483247 2147483647 1
400

chain 900 chrA 10000 + 1000 2000 next 5000 + 0 1000 2
1000
"""


def ascending(n):
    return [K(2200 + 5 * i, "s%d" % i) for i in range(n)]


def sets(W=8192):
    """name -> (chain text, records)"""
    out = {}
    for n in KEPT_EDGES:
        out["kept%d" % n] = (lc.CHAIN, interleave(scattered(n, 777 + n)))
    for n in (65, 257):
        recs = ascending(n)
        for i in range(0, n, 9):
            recs[i] = K(recs[max(i - 1, 0)]["pos"], "tie%d" % i)                  # (ties: a key equal to the one before is no descent)
        out["in_order%d" % n] = (lc.CHAIN, interleave(recs + [N("tail_a"), N("tail_b")]))
    for d in ONE_DESCENT_AT:
        recs = ascending(ONE_DESCENT_N); recs[d] = K(recs[d - 1]["pos"] - 3, "down%d" % d)
        out["one_descent%d" % d] = (lc.CHAIN, interleave(recs))
    out["equal"] = (lc.CHAIN, interleave([K(2500, "e%d" % i) for i in range(257)]))
    out["equal_desc"] = (lc.CHAIN, interleave([K(2500, "e%d" % i) for i in range(257)] + [K(2400, "low")] + [K(2500, "f%d" % i) for i in range(5)]))
    out["refid_only"] = (lc.CHAIN, interleave([K(5500, "B%d" % i, rid=1) if i % 2 == 0 else K(2250, "A%d" % i) for i in range(130)]))     # both lift to position 2500
    out["lowbit"] = (lc.CHAIN, interleave([K(2501 - i % 2, "l%d" % i) for i in range(130)]))
    recs = scattered(200, 4242)
    for i in range(3, 200, 17):
        recs[i] = N("none%d" % i)
    out["none_scattered"] = (lc.CHAIN, interleave(recs))
    out["big_pos"] = (BIG_CHAIN, interleave([K(1000 + 7 * i, "x%d" % i, cig=((1, "M"),)) if i % 2 == 0 else K(499 - i, "g%d" % i, cig=((1, "M"),)) for i in range(140)]))
    for name, recs in sorted(lc.walk_sets(W).items()):
        out["walk_" + name] = (lc.CHAIN, recs)
    for n in lc.SIZES:
        out["d%d" % n] = (lc.CHAIN, lc.directed(n))
    return out


def self_check(W=8192):
    """the sets do what their names say under the Python rules alone"""
    S = sets(W)
    for n in KEPT_EDGES:
        t = truth(*((S["kept%d" % n][0], lc.REFS, S["kept%d" % n][1])))
        assert len(t["perm"]) == n and (n < 3 or t["descents"] > 0), n
        assert all(p != i for i, p in enumerate(sorted(t["perm"]))), n          # compacted index != record index
    for n in (65, 257):
        t = truth(S["in_order%d" % n][0], lc.REFS, S["in_order%d" % n][1])
        assert t["descents"] == 0 and len(t["perm"]) == n + 2 and len(set(t["keys"])) < len(t["keys"]) and t["keys"][-1] == NONE
    for d in ONE_DESCENT_AT:
        chain, recs = S["one_descent%d" % d]; v, kept, _ = lc.lift_all(chain, lc.REFS, recs)
        ks = [key(k) for k in kept]
        assert [i for i in range(1, len(ks)) if ks[i] < ks[i - 1]] == [d] and len(ks) == ONE_DESCENT_N
    t = truth(S["equal"][0], lc.REFS, S["equal"][1]); assert len(set(t["keys"])) == 1 and len(t["keys"]) == 257 and t["perm"] == sorted(t["perm"])
    t = truth(S["equal_desc"][0], lc.REFS, S["equal_desc"][1]); assert t["descents"] == 1 and t["kept"][0]["qname"] == "low" and t["perm"][1:] == sorted(t["perm"][1:])
    t = truth(S["refid_only"][0], lc.REFS, S["refid_only"][1]); assert {k & 0xffffffff for k in t["keys"]} == {2500} and {k >> 32 for k in t["keys"]} == {0, 1} and t["descents"] > 60
    t = truth(S["lowbit"][0], lc.REFS, S["lowbit"][1]); assert {k for k in t["keys"]} == {2750, 2751} and t["descents"] > 60
    t = truth(S["none_scattered"][0], lc.REFS, S["none_scattered"][1]); n_none = t["keys"].count(NONE)
    assert n_none > 12 and t["keys"][-n_none:] == [NONE] * n_none and t["perm"][-n_none:] == sorted(t["perm"][-n_none:])
    t = truth(S["big_pos"][0], lc.REFS, S["big_pos"][1]); big = [k for k in t["keys"] if k >> 32 == 0]
    assert len(big) == 70 and min(big) >= (1 << 31) - 300 and max(big) < 1 << 31 and t["keys"][70] >> 32 == 1 and t["descents"] > 60
    t = truth(lc.CHAIN, lc.REFS, lc.directed(257))
    assert (len(t["perm"]), t["descents"], t["keys"].count(NONE), sorted({k >> 32 for k in t["keys"] if k != NONE})) == (156, 53, 24, [0, 1])
    return S

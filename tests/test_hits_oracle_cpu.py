"""The oracle's hit stage (o_frag_hits: gen_regs, set_parent, select_sub(_multi), seg_gen, squeeze_a, set_mapq of oracle/al_oracle.c) against the
reference's own functions (oracle/_ref/libhitref.so: hit.c and pe.c behind oracle/hitref_shim.c) on every directed fragment of tests/hits_cases.py
and under every option set; and the proof, on the reference's results alone, that the case list reaches what tests/test_gpu_hits_directed.py is
there to test: every chain-count class of k_regs_select and each of its bail-outs, every k_regs_heavy tile, the edges of the coverage bitmap, the
lists of k_map_only_wave, every MAPQ value and a log-table argument beyond the smallest table."""
import collections

import numpy as np
import pytest

import hits_cases as K

F = K.FIELDS.index


def same(a, b):
    return (len(a.A) == len(b.A) and np.array_equal(a.pre, b.pre) and np.array_equal(a.A, b.A) and len(a.B) == len(b.B)
            and all(np.array_equal(x, y) for x, y in zip(a.B, b.B)) and all(np.array_equal(x, y) for x, y in zip(a.C, b.C)) and all(np.array_equal(x, y) for x, y in zip(a.anch, b.anch)))


@pytest.mark.parametrize("optname", list(K.OPTION_SETS))
def test_oracle_equals_reference(optname):
    o = K.OPTION_SETS[optname]
    fr = K.cases(optname)
    hashes, want = K.reference(optname)
    orc = K.oracle_hits()
    bad = [K.describe(optname, f) for f, h, w in zip(fr, hashes, want) if not same(orc(o, f, h), w)]
    assert not bad, "%d of %d fragments differ\n%s" % (len(bad), len(fr), "\n".join(bad[:3]))
    ref = K.ref_hits()                                            # ... and on the fragments of 65535 and 65536 bases, which no batch can hold
    extra = K.host_only_cases(optname)
    assert len(extra) == 10 and all(sum(f.qlens) >= 65535 for f in extra)
    bad = [K.describe(optname, f) for f in extra if not same(orc(o, f, 12345), ref(o, f, 12345))]
    assert not bad, "\n".join(bad[:3])
    assert len(fr) > 800


def test_generator_is_deterministic_and_within_its_limits():
    for optname in K.OPTION_SETS:
        a = K.cases(optname)
        if optname in ("sr", "k28"):
            K._CACHE.pop(optname)
            b = K.cases(optname)
            assert len(a) == len(b) and all(x.label == y.label and x.qlens == y.qlens and x.rep_len == y.rep_len and np.array_equal(x.u, y.u) and np.array_equal(x.anchors, y.anchors) for x, y in zip(a, b))
        assert len(a) < 2000 and sum(len(f.anchors) for f in a) < 500000
        assert sum(1 for f in a if len(f.anchors) > 10000) == 2
        for f in a:                                               # every chain has anchors, and they add up
            assert int((f.u & np.uint64(0xffffffff)).sum()) == len(f.anchors) and (len(f.u) == 0 or int((f.u & np.uint64(0xffffffff)).min()) >= 1), f.label


def test_the_hash_is_the_one_of_the_name():
    fr = K.cases("sr")
    h = K.frag_hashes(fr)
    assert len(set(h)) > len(h) * 0.99 and h[0] != h[1]


@pytest.mark.parametrize("optname", ["sr", "best_n150", "pri_ratio0"])
def test_case_list_reaches_what_it_is_for(optname):
    o = K.OPTION_SETS[optname]
    fr = K.cases(optname)
    hashes, want = K.reference(optname)
    nu = [len(f.u) for f in fr]
    assert set(K.CHAIN_COUNTS) <= set(nu)
    # every chain-count class: below 5 (k_regs alone), 5-64, ... , above 8192
    cls = collections.Counter(sum(n >= e for e in K.CLASS_EDGES) for n in nu)
    assert all(cls[c] > 0 for c in range(len(K.CLASS_EDGES) + 1)), cls
    # every k_regs_heavy tile, and kept hits in its band that fit no tile
    tiles = collections.Counter(K.heavy_tile(w, n) for w, n in zip(want, nu))
    assert all(tiles[t] > 0 for t in range(6)), tiles
    kept = {K.kept_of(w)[0] for w in want}
    if o.pri_ratio > 0:
        assert {8, 9, 12, 13, 24, 25, 48, 49, 72, 73} <= kept, sorted(kept)
    if o.best_n >= 150:
        assert {200, 201} <= kept
    tot10 = {K.kept_of(w)[1] for w, f in zip(want, fr) if f.label.startswith("heavy ten kept")}
    if o.pri_ratio > 0:
        assert set(K.HEAVY_ANCHORS) <= tot10, sorted(tot10)
    # 64 primaries and more (REGS_PMAX)
    pr = [K.n_primaries(w) for w in want]
    assert pr.count(K.PMAX) > 0 and pr.count(K.PMAX - 1) > 0 and sum(p > K.PMAX for p in pr) > 0
    # the in-place compaction: aliased tests, the parent's old index on both sides of REGS_KCAP, inside one group of 64 sorted hits and across groups
    if o.pri_ratio > 0:
        al = [K.aliased(w) for w in want]
        assert sum(1 for a in al if a) >= 20
        ps = {p for a in al for p in a}
        assert any(p < K.KCAP - 1 for p in ps) and K.KCAP - 1 in ps and K.KCAP in ps and any(p > K.KCAP for p in ps), sorted(ps)
        assert any(p < 64 for p in ps) and any(64 <= p < K.KCAP for p in ps)
    # equal sort keys among at most 64 chains and among more; runs of more than 64 equal keys
    ties = [K.has_tie(f, h) for f, h in zip(fr, hashes)]
    assert sum(t and n <= 64 for t, n in zip(ties, nu)) >= 10 and sum(t and 64 < n <= 8192 for t, n in zip(ties, nu)) >= 10
    assert any("65 copies" in f.label for f in fr) and any("100 copies" in f.label for f in fr)
    # a score that does not fit 16 bits
    assert sum(1 for f in fr if len(f.u) >= 300 and int(f.u.max() >> np.uint64(32)) >= 65536) >= 4
    # the coverage bitmap's edge and the 16-bit query coordinates
    qs = {sum(f.qlens) for f in fr}
    assert {2048, 2049} <= qs and {(2048,), (2049,), (1024, 1024), (1025, 1024)} <= {f.qlens for f in fr}
    assert max(qs) == 2 * K.MAX_READ_LEN == 65534 and max(max(f.qlens) for f in fr) == K.MAX_READ_LEN   # the longest pair a batch can hold; beyond it: host_only_cases
    assert {sum(f.qlens) for f in K.host_only_cases(optname)} == {65535, 65536}
    # a mate without hits beside a mate with hits; mates of more than MO_LIGHT and of more than 64 hits
    assert sum(1 for w in want if len(w.B) == 2 and (len(w.B[0]) == 0) != (len(w.B[1]) == 0)) >= 10
    per_mate = collections.Counter(len(b) for w in want for b in w.B)
    if optname == "sr":
        assert all(per_mate[n] > 0 for n in (K.MO_LIGHT, K.MO_LIGHT + 1, 64, 65, 130)), per_mate
    assert any(n > 64 for n in per_mate)
    # every MAPQ, and an argument of logf beyond the smallest table
    mq = collections.Counter(int(v) for w in want for c in w.C for v in c[:, F("mapq")])
    assert all(mq[v] > 0 for v in range(61)) and max(mq) == 60, [v for v in range(61) if not mq[v]]
    assert max(int(c[:, F("n_sub")].max()) + 1 for w in want for c in w.C if len(c)) >= K.LOGTAB_N
    # nothing here sets the flag bits the stage leaves alone
    assert all(int((c[:, F("other")] != 0).sum()) == 0 for w in want for c in w.C)


def test_serial_subset_is_what_the_gpu_test_expects():
    """The all-serial configuration of the GPU test takes the fragments of at most SERIAL_MAX_CHAINS chains: everything but the largest classes."""
    fr = K.cases("sr")
    left_out = sorted({len(f.u) for f in fr if len(f.u) > K.SERIAL_MAX_CHAINS})
    assert left_out == [3000, 4096, 4097, 5000, 8192, 8193, 16500], left_out
    assert {2048, 2049} <= {len(f.u) for f in fr if len(f.u) <= K.SERIAL_MAX_CHAINS}

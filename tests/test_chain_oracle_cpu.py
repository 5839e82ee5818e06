"""The oracle's chaining (o_chain_dp, oracle/al_oracle.c) against the reference's mm_chain_dp, fragment by fragment, on the directed anchor
sets of tests/chain_cases.py: the number of chains, u[] in order and every chained anchor.  And the conditions under which that list proves,
with the reference alone, that it reaches the rules it names.  The whole-pipeline tests pin the oracle only where a difference moves a SAM line."""
import numpy as np
import pytest

import chain_cases as K


@pytest.fixture(scope="module")
def fns():
    return K.ref_chain(), K.oracle_chain()


_REF = {}


def reference(fns, optname):
    """[(u, chained)] of mm_chain_dp for K.cases(optname) (computed once)."""
    if optname not in _REF:
        o = K.OPTION_SETS[optname]
        _REF[optname] = [fns[0](o, f) for f in K.cases(optname)]
    return _REF[optname]


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("optname", list(K.OPTION_SETS))
def test_oracle_chaining_equals_reference(fns, optname):
    o = K.OPTION_SETS[optname]
    fr = K.cases(optname); ref = reference(fns, optname)
    bad = []; n = 0
    for f, r in zip(fr, ref):
        g = fns[1](o, f); n += 1
        if not same(g, r):
            bad.append("%s\n  oracle    %s\n  reference %s" % (K.describe(optname, f), K.chains_str(*g), K.chains_str(*r)))
            if len(bad) >= 4:
                break
    assert not bad, "\n".join(bad)
    assert n == len(fr) > 1000


def test_generator_is_deterministic_and_within_its_limits():
    fr = K.cases("sr")
    K._CACHE.pop("sr"); again = K.cases("sr")
    assert len(fr) == len(again) and all(a.label == b.label and a.qlens == b.qlens and a.tie == b.tie and np.array_equal(a.anchors, b.anchors) for a, b in zip(fr, again))
    for name in K.OPTION_SETS:
        c = K.cases(name)
        assert 1000 < len(c) < 6000 and max(len(f.anchors) for f in c) <= 9000 and sum(len(f.anchors) for f in c) < 400000
        for f in c:
            x = f.anchors[:, 0]
            assert (x[1:] >= x[:-1]).all(), f.label
            assert f.tie == bool((x[1:] == x[:-1]).any()), f.label
        assert {len(f.anchors) for f in c} >= set(K.FRAG_SIZES)
        assert {f.qlens for f in c} >= {(150, 150), (300,), (4095,), (2048, 2048), (350, 350), (350, 351), (349, 350)}
        # the pair sweep holds every dd in 0 ... bw + 1 on both sides, for the same mate and the other, alone and with the decoy
        ob = K.OPTION_SETS[name]
        labels = {f.label for f in c}
        for span in (K.SPANS if name == "sr" else (ob.k,)):
            for pre in ("pair", "pair+decoy"):
                for mate in ("same", "other"):
                    for side in ("r", "q"):
                        assert all("%s span%d %s dd%d side_%s" % (pre, span, mate, dd, side) in labels for dd in range(ob.bw + 2)), (name, span, pre, mate, side)
    o = K.OPTION_SETS
    assert o["min_cnt1"].min_chain_score <= o["min_cnt1"].k + 1                                   # lmin < 2
    assert max(o["max_gap40000"].max_gap, o["max_gap40000"].max_frag_len) > 0x7fff


@pytest.mark.parametrize("optname", list(K.OPTION_SETS))
def test_size_edges_are_in_what_the_reference_cuts_and_returns(fns, optname):
    """Every segment size, as a whole fragment and inside one -- by this file's own restatement of the cut rule (K.segments: chain.c:51 with
    the fragment's own max_dist_x), since the reference does not report segments; and, from mm_chain_dp itself, a chain out of a one-segment
    fragment of every size from min_cnt anchors on."""
    o = K.OPTION_SETS[optname]
    alone, inside, chained = set(), set(), set()
    for f, (u, ch) in zip(K.cases(optname), reference(fns, optname)):
        if not f.label.startswith("size "):
            continue
        sg = K.segments(o, f)
        (alone if len(sg) == 1 else inside).update(sg)
        if len(sg) == 1 and len(u):
            chained.add(sg[0])
    want = set(K.SEG_SIZES)
    assert want <= alone and want <= inside, (sorted(want - alone), sorted(want - inside))
    assert {n for n in want if n >= o.min_cnt} <= chained, sorted(want - chained)
    assert {n for n in K.FRAG_SIZES if n >= max(1, o.min_cnt)} <= chained


def test_chain_and_end_counts_are_what_the_reference_returns(fns):
    got_ends, got_chains = {}, {}
    for f, (u, ch) in zip(K.cases("sr"), reference(fns, "sr")):
        if f.label.startswith("ends ") and "chain ends in one segment" in f.label:
            assert len(K.segments(K.SR, f)) == 1
            got_ends[len(u)] = f.label
        if f.label.startswith("order ") and "tied starts" in f.label:
            assert K.tied_starts(u, ch), f.label
            got_chains.setdefault(len(u), []).append(len(K.segments(K.SR, f)))
    assert set(K.END_COUNTS) <= set(got_ends), got_ends
    assert set(K.CHAIN_COUNTS) <= set(got_chains), got_chains
    for n, segs in got_chains.items():
        assert 1 in segs and max(segs) > 1, (n, segs)                                             # in one segment, and in segments of 16 chains


def test_at_least_fifty_fragments_have_tied_chain_starts(fns):
    n = sum(1 for u, ch in reference(fns, "sr") if K.tied_starts(u, ch))
    assert n >= 50, n
    many = sum(1 for u, ch in reference(fns, "sr") if len(u) > 64 and K.tied_starts(u, ch))
    few = sum(1 for u, ch in reference(fns, "sr") if 2 <= len(u) <= 64 and K.tied_starts(u, ch))
    assert many >= 5 and few >= 5, (many, few)


@pytest.mark.parametrize("optname", ["sr", "skip0", "skip5", "skip6", "skip7"])
def test_max_skip_bites_on_the_dense_fragments(fns, optname):
    o = K.OPTION_SETS[optname]
    d = [(f, r) for f, r in zip(K.cases(optname), reference(fns, optname)) if f.label.startswith("dense ")]
    differ = sum(1 for f, r in d if not same(fns[0](o, f, max_skip=1 << 30), r))
    assert len(d) >= 40 and differ * 4 >= len(d), "max_chain_skip %d changes %d of %d dense fragments" % (o.max_chain_skip, differ, len(d))


@pytest.mark.parametrize("optname", ["iter128", "iter127"])
def test_max_iter_bites_on_the_dense_fragments(fns, optname):
    o = K.OPTION_SETS[optname]
    d = [(f, r) for f, r in zip(K.cases(optname), reference(fns, optname)) if f.label.startswith("dense ")]
    differ = sum(1 for f, r in d if not same(fns[0](o, f, max_iter=5000), r))
    assert len(d) >= 40 and differ * 4 >= len(d), "max_chain_iter %d changes %d of %d dense fragments" % (o.max_chain_iter, differ, len(d))


@pytest.mark.parametrize("optname", ["sr", "min_cnt3_sc40", "k15"])      # (k 28, min_cnt 1: a chain of min_cnt anchors is above min_chain_score at once)
def test_filters_are_reached_on_both_sides(fns, optname):
    """min_chain_score on a lone chain's score and on what a branch adds to the chain it runs into, min_cnt, and a peak before the chain's end."""
    o = K.OPTION_SETS[optname]
    lone, branch, peak = {}, {}, []
    for f, (u, ch) in zip(K.cases(optname), reference(fns, optname)):
        w = f.label.split()
        if f.label.startswith("ends lone chain of"):
            m, last = int(w[4].rstrip(",")), int(w[-1])
            lone[(m, last)] = (len(u), int(u[0] >> np.uint64(32)) if len(u) else -1, int(u[0] & np.uint64(0xffffffff)) if len(u) else 0)
        elif f.label.startswith("ends branch of"):
            nb, last = int(w[3].rstrip(",")), int(w[-1])
            branch[(nb, last)] = sorted(int(x >> np.uint64(32)) for x in u)
        elif f.label.startswith("ends peak before end"):
            peak.append((len(f.anchors), [int(x & np.uint64(0xffffffff)) for x in u]))
    # a lone chain: kept with a score of exactly min_chain_score, dropped one step shorter
    sc = o.min_chain_score
    kept = [k for k, v in lone.items() if v[0] == 1 and v[1] == sc and v[2] >= o.min_cnt]
    assert kept and all(lone.get((m, last - 1), (0,))[0] == 0 for m, last in kept), (sc, lone)
    # min_cnt: a chain of min_cnt anchors is kept, one of min_cnt - 1 anchors with a score that would pass is not
    assert any(v[0] == 1 and v[2] == o.min_cnt for v in lone.values())
    if o.min_cnt > 1 and (o.min_cnt - 1) * o.k >= sc:
        assert all(v[0] == 0 for (m, last), v in lone.items() if m == o.min_cnt - 1)
    # a branch that runs into the longer chain: kept when it adds exactly min_chain_score, dropped when it adds one less
    top = max(max(v) for v in branch.values() if v)
    two = {k: v for k, v in branch.items() if len(v) == 2}
    on = [k for k, v in two.items() if v[0] == sc and v[1] == top]
    assert on, (sc, branch)
    assert any(len(branch[(nb, last - 1)]) == 1 for nb, last in on if (nb, last - 1) in branch), branch
    # the peak is not the end: every anchor is linked, the chain stops before the last one
    assert peak and all(len(c) == 1 and c[0] == n - 1 for n, c in peak), peak

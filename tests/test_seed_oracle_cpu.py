"""The oracle's sketch and seeding (o_sketch, o_collect_seeds, oidx_build of oracle/al_oracle.c) against the reference's (mm_sketch, mm_idx_str and
the static collect_minimizers / collect_seed_hits_heap of map.c, oracle/_ref/libseedref.so) on the directed cases of tests/seed_cases.py: the
minimizers of every read, and of every fragment and pass the anchors in order, rep_len and the counts.  And the census: the conditions under which
that list proves, with the reference's results alone, that it holds the sizes, ties, list counts, list lengths, strands, positions, lookup edges
and index shapes it names -- what keeps tests/test_gpu_seed_directed.py, which runs the same cases through the kernels, from being vacuous."""
import os
import time

import numpy as np
import pytest

import seed_cases as K

U64 = np.uint64
LARGE = ("c32768", "c32769", "c65536", "c65537")


@pytest.fixture(scope="module")
def oracle():
    return K.Oracle()


def results(name):
    ref, frags, second = K.case_set(name)
    res, mini, occ = K.reference_results(name)
    return ref, frags, second, res, mini, occ


def passes(ref, res):
    """[(pass, bound, [(fragment index, Res)])]"""
    return [(1, ref.shape.mid_occ, [(i, r[0]) for i, r in enumerate(res)]), (2, ref.shape.max_occ, [(i, r[1]) for i, r in enumerate(res) if r[1] is not None])]


@pytest.mark.parametrize("name", list(K.SHAPES))
def test_oracle_seeding_equals_reference(oracle, name):
    ref, frags, second, res, mini, occ = results(name)
    sh = ref.shape
    h = oracle.index(sh.k, sh.w, ref.contigs, ref.names)
    bad = []; n = 0
    for f, (r1, r2), mv in zip(frags, res, mini):
        for r, bound in ((r1, sh.mid_occ), (r2, sh.max_occ)):
            if r is None:
                continue
            a, rep = oracle.frag(h, f.seqs, bound)
            if len(a) != r.n_a or rep != r.rep_len or not np.array_equal(a, r.anchors):
                bad.append("%s (bound %d): oracle %d anchors, rep_len %d; reference %d, %d" % (f.label, bound, len(a), rep, r.n_a, r.rep_len))
        for s, m in zip(f.seqs, mv):
            if not np.array_equal(oracle.sketch(s, sh.w, sh.k), m):
                bad.append("%s: minimizers differ" % f.label)
        n += 1
    oracle.destroy(h)
    assert not bad, "\n".join(bad[:6])
    assert n == len(frags) > 0 and second == [i for i, f in enumerate(frags) if f.second] and len(second) > 0


@pytest.mark.parametrize("k,w", K.SKETCH_SETS)
def test_oracle_sketch_equals_reference(oracle, k, w):
    R = K.seedref()
    reads = K.sketch_reads(k, w)
    some = 0
    for label, s in reads:
        want = R.sketch(s, w, k)
        assert np.array_equal(oracle.sketch(s, w, k), want), (k, w, label)
        some += len(want) > 0
    lens = {len(s) for _, s in reads}
    assert lens >= {0, 1, k - 1, k, k + w - 2, k + w - 1, k + w, 7, 8, 9, 15, 16, 17, 150, 250} and some > 50
    if (k, w) == (25, 11):
        assert {8191, 8192} <= lens
    # tied minima inside a window (homopolymer, (AC)n): more minimizers than windows would give one each
    labels = dict(reads)
    for nm in ("homopolymer 150", "AC 150"):
        assert len(R.sketch(labels[nm], w, k)) >= (1 if k % 2 == 0 and nm.startswith("AC") else 2) or w == 1, (nm, k, w)
    assert len(R.sketch(labels["all N 150"], w, k)) == 0
    if k % 2 == 0:                                                           # (AT)n: every k-mer is its own reverse complement at even k, none is kept
        assert len(R.sketch(labels["AT 150"], w, k)) == 0
    if k % 4 == 0:                                                           # (ACGT)n: one k-mer in four is, the window does not move for it
        assert 0 < len(R.sketch(labels["ACGT 150"], w, k))


@pytest.fixture(scope="module")
def A():
    import airlift_amd
    if not os.path.exists(airlift_amd.lib_path()):
        airlift_amd.build()
    airlift_amd.load()
    return airlift_amd


@pytest.mark.parametrize("name", LARGE + ("c3",))
def test_host_index_holds_the_oracles_occurrence_array(A, oracle, name):
    ref = K.case_set(name)[0]
    sh = ref.shape
    idx = A.Index(seqs=ref.contigs, names=ref.names, k=sh.k, w=sh.w)
    h = oracle.index(sh.k, sh.w, ref.contigs, ref.names)
    got = idx.positions(); want, n_keys = oracle.positions_by_key(h)
    st = idx.stat()
    assert st["n_pos"] == len(want) == h.contents.n_pos and st["n_keys"] == h.contents.n_keys == n_keys and st["n_bases"] == sum(len(c) for c in ref.contigs)
    assert len(idx.names) == sh.n_contigs
    oracle.destroy(h); idx.close()
    # the host index exports its lists in ascending order of their keys, positions ascending inside a list: the oracle's lists, taken key by key in that
    # order, must give the same array -- a position filed under another key, or a list cut elsewhere, moves an element
    assert np.array_equal(got, want)


def test_generator_is_deterministic_and_within_its_limits():
    for name in K.SHAPES:                                                   # every case set: the same twice, each time in under 20 s
        ref, frags, second = K.case_set(name)
        for key in (name, ("results", name)):
            K._CACHE.pop(key, None)
        t = time.time()
        ref2, frags2, second2 = K.case_set(name)
        K.reference_results(name)
        assert time.time() - t < 20, name
        assert ref.contigs == ref2.contigs and frags == frags2 and second == second2, name
    for name in K.SHAPES:
        ref, frags, second, res, mini, occ = results(name)
        assert len(frags) < 4000
        assert sum(r1.n_a + (r2.n_a if r2 is not None else 0) for r1, r2 in res) < 2500000
        assert sum(len(c) for c in ref.contigs) < 5000000 and len(ref.contigs) == ref.shape.n_contigs
        assert max(len(s) for f in frags for s in f.seqs) < 8192


def rid_of(x):
    return (x << U64(1)) >> U64(33)


def pos_of(x):
    return x & U64(0xffffffff)


@pytest.mark.parametrize("name", [n for n, s in K.SHAPES.items() if not s.long_list])
def test_census_sizes_and_ties(name):
    """Every anchor count of the ladder, in the first pass and in the re-chain pass, untied and (from 2 anchors) tied."""
    ref, frags, second, res, mini, occ = results(name)
    sizes = K.SIZES if ref.shape.full else tuple(n for n in K.SIZES if n <= 2049)
    for p, bound, rs in passes(ref, res):
        have = {(r.n_a, r.tied) for _, r in rs}
        for n in sizes:
            assert (n, False) in have, (name, p, n)
            assert n < 2 or (n, True) in have, (name, p, n, "tied")
        assert not any(r.tied for _, r in rs if r.n_lists < 2)                # (no tie inside one list)


def test_census_giant_caps_lists_and_lengths():
    ref, frags, second, res, mini, occ = results("c3")
    for p, bound, rs in passes(ref, res):
        for tied in (False, True):                                          # several passes of the run merge at the default run length of 8192: more than 2 * 8192 anchors
            assert any(r.n_a >= K.GIANT and r.tied == tied and r.n_lists <= 1024 for _, r in rs), (p, tied)
        for m in K.TIED_LIST_COUNTS:
            assert any(r.tied and r.n_lists == m for _, r in rs), (p, m)
        for c in K.TIED_LIST_LENGTHS:
            assert any(r.tied and (r.lists == c).sum() >= 2 for _, r in rs), (p, c)
        assert any(r.tied and 1 <= r.n_lists <= 63 for _, r in rs) and any(r.tied and 64 <= r.n_lists <= 126 for _, r in rs) and any(r.tied and r.n_lists > 126 for _, r in rs)
        assert any(r.tied and r.n_lists > 512 for _, r in rs)
        for n_lists, _, a_lo, a_hi in K.CAP_CASES:
            assert any(not r.tied and r.n_lists == n_lists and a_lo <= r.n_a <= a_hi for _, r in rs), (p, n_lists, a_lo)
    ref, frags, second, res, mini, occ = results("c3_long")
    rs = passes(ref, res)[1][2]
    assert any(r.tied and (r.lists >= 2000).sum() >= 2 for _, r in rs) and any(not r.tied and (r.lists >= 2000).any() for _, r in rs)
    assert any(r.tied and (r.lists >= 2000).any() and len(frags[i].seqs) == 2 for i, r in rs)


def test_census_strands_and_positions():
    ref, frags, second, res, mini, occ = results("c3")
    lens = [len(c) for c in ref.contigs]
    for p, bound, rs in passes(ref, res):
        big = [r for _, r in rs if r.n_a >= 20]
        assert any(r.n_rev == 0 for r in big) and any(r.n_rev == r.n_a for r in big) and any(0 < r.n_rev < r.n_a for r in big)
        assert {r.n_rev % 2 for _, r in rs if r.n_rev > 2} == {0, 1}            # the reversal loop of map.c:202-207, with and without a middle element
        allx = np.concatenate([r.anchors[:, 0] for _, r in rs])
        rid, pos = rid_of(allx), pos_of(allx)
        assert ((rid == U64(ref.longest)) & (pos == U64(lens[ref.longest] - 1))).any()       # the last base of the longest contig
        assert (rid == U64(len(lens) - 1)).any() and (rid == U64(0)).any()
        on_two = opposite = False
        for _, r in rs:
            x = r.anchors[:, 0]
            if len(x) < 2 or len(x) > 500:
                continue
            key = set(zip(rid_of(x).tolist(), pos_of(x).tolist(), (x >> U64(63)).tolist()))
            on_two = on_two or any((rr ^ 1, pp, ss) in key for rr, pp, ss in key if rr < 2)
            opposite = opposite or (not r.tied and any((rr, pp, 1 - ss) in key for rr, pp, ss in key))
        assert on_two and opposite, (p, on_two, opposite)


def filtered(mv_frag, seqs, occ, bound):
    """Per minimizer of the fragment, in collect_minimizers' order: (position in the fragment, segment, hash, occurrences)."""
    out = []; tot = 0
    for seg, (m, s) in enumerate(zip(mv_frag, seqs)):
        for x, y in m.tolist():
            out.append(((int(y) & 0xffffffff) // 2 + tot, seg, x >> 8, occ[x >> 8]))
        tot += len(s)
    return out


def test_census_seed_lookup():
    ref, frags, second, res, mini, occ = results("c3")
    k = ref.shape.k
    assert {len(m) % 4 for mv in mini for m in mv} == {0, 1, 2, 3}
    assert any(len(mv) == 1 and len(mv[0]) == 0 for mv in mini)
    assert any(len(mv) == 2 and len(mv[1]) == 0 and len(mv[0]) > 0 for mv in mini) and any(len(mv) == 2 and len(mv[0]) == 0 and len(mv[1]) > 0 for mv in mini)
    for p, bound, rs in passes(ref, res):
        lists = np.concatenate([r.lists for _, r in rs])
        assert (lists == bound - 1).any() and (lists == 0).any() and (lists == 1).any() and (lists == 2).any() and (lists == 3).any() and not (lists >= bound).any()
        gaps = set(); across = set(); first = last = False; runs = set(); run_at = set(); run_across = run_filtered = False; flagged = 0
        occs = set()
        for i, r in rs:
            mm = filtered(mini[i], frags[i].seqs, occ, bound)
            occs.update(o for _, _, _, o in mm)
            f = [(q, seg) for q, seg, _, o in mm if o >= bound]
            for (q0, s0), (q1, s1) in zip(f, f[1:]):
                d = q1 - q0
                cls = "overlap" if d < k else "touching" if d == k else "one apart" if d == k + 1 else "disjoint"
                gaps.add(cls)
                if s0 != s1:
                    across.add(cls)
            if mm and f:
                first = first or mm[0][3] >= bound; last = last or mm[-1][3] >= bound
            # runs of equal neighbouring hashes over the whole list
            j = 0; per_seg_start = {}
            idx_in_seg = []; c = {}
            for q, seg, hsh, o in mm:
                idx_in_seg.append(c.get(seg, 0)); c[seg] = c.get(seg, 0) + 1
            while j < len(mm):
                e = j
                while e + 1 < len(mm) and mm[e + 1][2] == mm[j][2]:
                    e += 1
                if e > j:
                    kept = 0 < mm[j][3] < bound
                    if kept:
                        runs.add(min(e - j + 1, 4)); run_at.add(idx_in_seg[j] % 4)
                        run_across = run_across or mm[j][1] != mm[e][1]
                    run_filtered = run_filtered or mm[j][3] >= bound
                j = e + 1
            flagged += int(((r.anchors[:, 1] & U64(K.TANDEM)) != 0).any())
        assert bound in occs and bound - 1 in occs, (p, sorted(o for o in occs if o > 40)[:20])   # occurrence counts of exactly the bound (filtered) and one below (kept)
        assert gaps == {"overlap", "touching", "one apart", "disjoint"}, (p, gaps)
        assert {"touching", "disjoint"} <= across, (p, across)               # (an interval cannot overlap the other mate's: a minimizer ends at least k bases into its read)
        assert first and last, p
        assert {2, 3} <= runs and run_at == {0, 1, 2, 3} and run_across and run_filtered, (p, runs, run_at, run_across, run_filtered)
        assert flagged >= 20, (p, flagged)
        assert any(r.rep_len > 0 for _, r in rs) and any(r.rep_len == 0 and r.n_a > 0 for _, r in rs)


@pytest.mark.parametrize("name", LARGE + ("c1", "c2", "c3"))
def test_census_index_shapes(name):
    ref, frags, second, res, mini, occ = results(name)
    n = ref.shape.n_contigs
    assert len(ref.contigs) == n == int(name[1:])
    for p, bound, rs in passes(ref, res):
        once = set(); anyrid = set()
        for i, r in rs:
            rid = set(rid_of(r.anchors[:, 0]).tolist())
            anyrid |= rid
            if r.n_a and (r.lists <= 1).all():                              # anchors of once-occurring minimizers only
                once |= rid
        want = {0, n - 1} | ({32768} if n > 32768 else set()) | ({65536} if n > 65536 else set())
        assert want <= anyrid, (name, p, sorted(want - anyrid))
        assert want <= once, (name, p, sorted(want - once))

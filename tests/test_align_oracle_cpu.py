"""The oracle's extension half (o_frag_align: align_regs with align_skeleton / align1 / update_extra / filter_regs / hit_sort, set_mapq, pair_regs) against the
reference's own functions (oracle/_ref/libalignref.so: map.c:379-405 behind oracle/alignref_shim.c) on every directed fragment of tests/align_cases.py
under every option set, record by record, field by field and CIGAR word by CIGAR word -- and the proof, on the reference alone, that the lists reach what
they are written for.  Where the reference's records show the reach (split bits, hit counts that dropped, n_cigar, proper_frag, pe_thru, MAPQ) it is
taken from them; which branch of mm_align1 ran is taken from the counters of the oracle, which the comparison has just pinned.

Not as one might expect: under `sr` mm_test_zdrop never returns 2 (align.c:72 excludes MM_F_SR), so no record carries inv or split_inv and mm_align1_inv
never inserts one -- asserted below as zeros.  sr's max_clip_ratio of 1.0 never lets the clip filter of mm_filter_regs fire: the option set clip02 lowers it."""
import numpy as np
import pytest

import align_cases as K

SETS = list(K.OPTION_SETS)
_STATE = {}


def _run(optname):
    """(fragments, reference results, oracle results, the oracle's branch counters) of an option set: cases, long-mode list and arena list together."""
    if optname not in _STATE:
        o = K.OPTION_SETS[optname]
        fr, want = [], []
        for which, lst in (("cases", K.cases(optname)), ("long", K.long_cases(optname)), ("arena", K.arena_cases(optname))):
            fr += [(which, i, f) for i, f in enumerate(lst)]; want += K.reference(optname, which)[1]
        orc = K.oracle_align(o.k); cnt = np.zeros(len(K.AC), dtype=np.int64)
        hashes = {w: K.reference(optname, w)[0] for w in ("cases", "long", "arena")}
        K.oracle_count(cnt)
        try:
            got = [orc(o, f, hashes[w][i]) for w, i, f in fr]
        finally:
            K.oracle_count(None)
        _STATE[optname] = (fr, want, got, dict(zip(K.AC, cnt.tolist())))
    return _STATE[optname]


@pytest.mark.parametrize("optname", SETS)
def test_oracle_equals_reference(optname):
    fr, want, got, _ = _run(optname)
    bad = []
    for (w_, i, f), w, g in zip(fr, want, got):
        for s in range(len(f.qlens)):
            if w.hits[s].shape != g.hits[s].shape:
                bad.append("%s\n  mate %d: %d records, the reference %d" % (K.describe(optname, f), s, len(g.hits[s]), len(w.hits[s]))); break
            if not np.array_equal(w.hits[s], g.hits[s]):
                h, c = (int(x[0]) for x in np.nonzero(w.hits[s] != g.hits[s]))
                bad.append("%s\n  mate %d record %d: %s is %d, the reference's %d" % (K.describe(optname, f), s, h, K.FIELDS[c], g.hits[s][h, c], w.hits[s][h, c])); break
            if any(not np.array_equal(a, b) for a, b in zip(w.cigars[s], g.cigars[s])):
                bad.append("%s\n  mate %d: a CIGAR differs" % (K.describe(optname, f), s)); break
    print("[%s] %d fragments compared" % (optname, len(fr)))
    assert len(fr) > 1000 and not bad, "%d fragments differ\n%s" % (len(bad), "\n".join(bad[:4]))


def _reach(optname):
    """What an option set's lists reach, from the reference's records, the fragments themselves and the oracle's branch counters."""
    o = K.OPTION_SETS[optname]
    fr, want, _, cnt = _run(optname)
    C_ = K.COL; r = dict(cnt)
    allh = np.concatenate([h for w in want for h in w.hits if len(h)])
    ncig = allh[:, C_["n_cigar"]]
    r["records"] = len(allh)
    r["inv_or_split_inv"] = int((allh[:, C_["inv"]] | allh[:, C_["split_inv"]] | allh[:, C_["trans_strand"]]).sum())
    r["split_left"] = int((allh[:, C_["split"]] & 1).sum()); r["split_right"] = int((allh[:, C_["split"]] >> 1 & 1).sum())
    for n in (K.FCIG - 1, K.FCIG + 1):
        r["n_cigar_%d" % n] = int((ncig == n).sum())
    r["n_cigar_32"] = int((ncig == K.FCIG).sum())
    r["n_cigar_above_fcig"] = int((ncig > K.FCIG).sum()); r["n_cigar_above_inline"] = int((ncig > K.CIG_INLINE).sum()); r["n_cigar_1"] = int((ncig == 1).sum())
    r["proper_frag"] = int(allh[:, C_["proper_frag"]].sum()); r["pe_thru"] = int(allh[:, C_["pe_thru"]].sum())
    r["dp_max2"] = int((allh[:, C_["dp_max2"]] > 0).sum()); r["n_ambi"] = int((allh[:, C_["n_ambi"]] > 0).sum())
    r["dp_max_above_dp_score"] = int((allh[:, C_["dp_max"]] > allh[:, C_["dp_score"]]).sum())
    r["gaps_in_blen"] = int((allh[:, C_["blen"]] > allh[:, C_["mlen"]]).sum())
    r["at_min_dp_max"] = int((allh[:, C_["dp_max"]] == o.min_dp_max).sum() + (allh[:, C_["dp_max"]] == o.min_dp_max + 1).sum())
    r["mapq_values"] = len(set(allh[:, C_["mapq"]].tolist())); r["mapq_60"] = int((allh[:, C_["mapq"]] == 60).sum()); r["mapq_0_primary"] = int(((allh[:, C_["mapq"]] == 0) & (allh[:, C_["id"]] == allh[:, C_["parent"]])).sum())
    r["secondary"] = int((allh[:, C_["id"]] != allh[:, C_["parent"]]).sum()); r["rev"] = int(allh[:, C_["rev"]].sum()); r["fwd"] = len(allh) - r["rev"]
    lost_all = dropped = unpaired = one_anchor = sam_pri_not_first = swapped = 0; per_mate = {}; core_lens = set(); tiles = set(); most = 0
    for (w_, i, f), w in zip(fr, want):
        cntc = (f.u & np.uint64(0xffffffff)).astype(np.int64); off = np.concatenate([[0], np.cumsum(cntc)])
        one_anchor += int((cntc == 1).sum())
        for c in range(len(cntc)):
            a = f.anchors[off[c]:off[c + 1]]; seg = (a[:, 1] >> np.uint64(48)) & np.uint64(0xff)
            for s in set(seg.tolist()):
                b = a[seg == s]; dq = np.diff(b[:, 1].astype(np.int64) & 0xffffffff); dr = np.diff(b[:, 0].astype(np.int64) & 0xffffffff)
                if len(b) and np.array_equal(dq, dr):
                    core_lens.add(int(b[-1, 1] & np.uint64(0xffffffff)) - int(b[0, 1] & np.uint64(0xffffffff)) + int(b[0, 1] >> np.uint64(32) & np.uint64(0xff)))
        n = [len(h) for h in w.hits]
        lost_all += len(cntc) > 0 and sum(n) == 0
        dropped += sum(n) < len(cntc)
        unpaired += len(n) == 2 and min(n) == 0 < max(n)
        most = max(most, max(n))
        for h in w.hits:
            per_mate[len(h)] = per_mate.get(len(h), 0) + 1
            sam_pri_not_first += len(h) > 1 and int(h[0, C_["sam_pri"]]) == 0
            # a primary with a smaller chaining score than one of its secondaries: before alignment the hits lay in the order of that score, so the sort by dp_max moved the parent
            par = h[:, C_["parent"]]; sec = np.nonzero((par != h[:, C_["id"]]) & (par >= 0) & (par < len(h)))[0]
            swapped += bool(len(sec)) and bool((h[sec, C_["score"]] > h[par[sec], C_["score"]]).any())
        tiles.add(K.tile_of(o, max(f.qlens)))
    r.update(fragments=len(fr), lost_all=int(lost_all), hits_dropped=int(dropped), one_mate_unmapped=int(unpaired), chains_of_one_anchor=int(one_anchor), sam_pri_moved=int(sam_pri_not_first), most_hits=int(most), parent_changed_by_sort=int(swapped))
    r["core_lengths_1_to_40"] = len(core_lens & set(range(1, 41)))
    for n in (1, 3, 4, 12, 20):
        r["mates_of_%d_hits" % n] = per_mate.get(n, 0)
    r["mates_above_best_n"] = sum(v for k, v in per_mate.items() if k > o.best_n)
    r["tiles"] = sorted(tiles)
    return r


# every item must be reached (> 0) under sr; the other sets: what they are named for
SR_ITEMS = ("win_grown", "win_plain", "win_left_at0", "win_left_cut", "win_right_at_end", "win_right_cut", "stretch_first", "stretch_mid", "stretch_last", "chains_of_one_anchor",
            "left", "right", "reach_end", "clipped", "flank_zdrop", "flank_empty", "core_zdrop", "core_second_pass_kept", "split", "drop_no_split", "split_left", "split_right",
            "n_cigar_1", "n_cigar_31", "n_cigar_32", "n_cigar_33", "cigar_merged", "cigar_not_merged", "fall_eq_zdrop", "fall_zdrop_plus1", "tie_eq", "tie_above", "select_dropped",
            "flt_mlen", "flt_dp", "flt_dp_just_below", "kept_at_min_dp", "parent_changed_by_sort", "n_cigar_above_fcig", "n_cigar_above_inline", "proper_frag", "pe_thru", "dp_max2", "n_ambi", "dp_max_above_dp_score", "gaps_in_blen",
            "at_min_dp_max", "mapq_60", "mapq_0_primary", "secondary", "rev", "fwd", "lost_all", "hits_dropped", "one_mate_unmapped", "sam_pri_moved",
            "mates_of_1_hits", "mates_of_3_hits", "mates_of_4_hits", "mates_of_12_hits", "mates_above_best_n")
NAMED_FOR = {
    "end_bonus0": ("clipped", "win_plain", "flank_empty"),            # (without a bonus ksw_extd2 never reports reach_end)
    "zdrop30": ("core_zdrop", "split", "drop_no_split", "flank_zdrop"),
    "min_dp_max100": ("hits_dropped", "lost_all", "at_min_dp_max"),
    "best_n1": ("secondary",),
    "no_closed_form": ("left", "right", "reach_end", "clipped"),
    "bw10": ("flank_zdrop", "clipped"),
    "clip02": ("flt_clip", "flt_clip_just_above", "kept_clip_at_bound"),
}


@pytest.mark.parametrize("optname", SETS)
def test_case_list_reaches_what_it_is_written_for(optname):
    o = K.OPTION_SETS[optname]
    r = _reach(optname)
    print("[%s] reach: %s" % (optname, ", ".join("%s %s" % kv for kv in r.items())))
    assert r["inv_or_split_inv"] == 0                                    # unreachable under sr (align.c:72)
    assert r["core_lengths_1_to_40"] == 40
    assert r["tiles"] == [0, 336, 512, 1024]                              # a batch for each k_align instance and one for k_align_long
    assert K.tile_edges(K.SR) == [160, 161, 248, 249, 504, 505] and set(K.tile_edges(o)) <= set(max(f.qlens) for _, _, f in _run(optname)[0])
    for k in (SR_ITEMS if optname == "sr" else NAMED_FOR[optname]):
        assert r[k] > 0, "the list of %s does not reach %s: %s" % (optname, k, r)
    if optname == "best_n1":
        assert r["most_hits"] <= 2 and r["mates_above_best_n"] > 0
    if optname == "no_closed_form":
        assert not o.a + o.b < min(o.q + o.e, o.q2 + o.e2)
    else:
        assert o.a + o.b < min(o.q + o.e, o.q2 + o.e2)
    if optname == "min_dp_max100":
        assert r["hits_dropped"] > _reach("sr")["hits_dropped"]
    if optname == "zdrop30":
        assert r["core_zdrop"] > _reach("sr")["core_zdrop"] - 1 and r["split"] > 0

"""The kernels of the extension stage -- k_ext_prep(_wave), the DP job classes, k_ext_finish(_wave), the monolithic k_align<336|512|1024> and
k_align_long with their early, late and solo launches, k_compact, the arena-overflow re-run -- against the reference's path from a mate's hits to its
final records (oracle/_ref/libalignref.so: mm_align_skeleton with mm_align1, mm_update_extra, mm_filter_regs, mm_hit_sort; mm_set_parent, mm_select_sub,
mm_set_sam_pri; mm_set_mapq; mm_pair), fragment by fragment, mate by mate and record by record, on the directed fragments of tests/align_cases.py: the
record count, every record's id, parent, score, score0, cnt, rid, qs, qe, rs, re, subsc, n_sub, hash, mlen, blen, mapq, every flag (rev, split, inv,
split_inv, proper_frag, pe_thru, sam_pri, seg_split, seg_id), dp_score, dp_max, dp_max2, n_ambi, n_cigar and every CIGAR word.  Integer equality
throughout; the reference values are computed by the library on the spot.

The fragments go through al_dbg_align -- al_run_align_stage itself, to its end -- each configuration in a fresh process
(tests/helpers/align_directed_child.py: the environment switches are read once per process) under a time limit of its own; after a child that ended on
a signal or at its limit no further child is started.

Measured on an MI355X: a configuration's child takes about 1.2 s of wall time, of which the case list and the reference take 0.2 s and the stage's 24
calls with their fetches 0.4 s (the rest: imports, the index, the context); all twenty configurations ran in 26.2 s.  The long-mode list (a dozen reads
of 2 000 bases, k_align_long) and the arena-overflow list have configurations of their own.  Each child gets 120 s.

wave_prep and wave_finish are not counted by the wave kernels: the tap counts, from the job table the run left, the fragments at or above the threshold
the host passed to them -- the kernels' own rule restated on the host -- and the finish count includes fragments already on the early slow list, which
k_ext_finish_wave skips.

Not as one might expect: mm_test_zdrop never returns 2 under sr (align.c:72), so there is no inversion to test; the batch of 505-base reads, one base
beyond the largest tile, is in long mode already, so the plain list holds one k_align_long batch; with zdrop below b + max(q + e, q2 + e2) the kernels
take no closed form (d_ext_prep_frag's own rule), so the zdrop30 set asserts a closed-form count of 0; a wave-form fragment's first slow hit is hit
0, 1 or its last of 12 or 13 (best_n keeps 21 hits a mate at the most, so hit 63 does not exist)."""
import json
import os
import subprocess
import sys

import pytest

import align_cases as K

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "align_directed_child.py")
SWITCHES = ("AL_DBG", "AL_DBG2", "AL_PREP_HEAVY", "AL_FIN_HEAVY", "AL_DP_EXIT", "AL_DP_PK", "AL_DP_PK32", "AL_DP_EXIT_STRIDE", "AL_TEST_SCRUB", "AL_TEST_GUARD", "AL_TEST_POISON", "AL_DBG_FRAG")
LIMIT = 120                                                               # seconds for a child: a wide margin over the measured times above
FAST = ("wave_prep", "wave_finish", "closed_form", "n_jobs", "n_early", "n_slow")
_stop = []                                                                # why no further child is started


def run_child(optname, which, env):
    if _stop:
        pytest.fail("not run: %s" % _stop[0])
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env)
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable, CHILD, optname, which], capture_output=True, env=e)
    err = r.stderr.decode()
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _stop.append("the child of [%s %s, %s] ended with status %d" % (optname, which, env, r.returncode))
    assert r.returncode == 0, "[%s %s, %s] exit status %d\n%s\n%s" % (optname, which, env, r.returncode, r.stdout.decode()[-3000:], err[-3000:])
    res = json.loads(r.stdout.decode().strip().split("\n")[-1])
    print("[%s %s %s] %.1f s (cases and reference %.1f s, the stage's calls and fetches %.1f s)" % (optname, which, env, res["seconds"], res["seconds_cases"], res["seconds_stage"]))
    assert res["n_mismatch"] == 0, "[%s %s, %s] %d fragments differ\n%s" % (optname, which, env, res["n_mismatch"], "\n".join(res["mismatches"]))
    n = {"cases": K.cases, "long": K.long_cases, "arena": K.arena_cases}[which](optname)
    assert res["compared"] == res["generated"] == len(n)                   # nothing skipped or filtered out after generation
    assert res["counts"]["log_miss"] == 0 and res["counts"]["limit"] == 0 and res["counts"]["arena_overflow"] == 0   # no bail-out word left behind
    assert not res["tile_wrong"], "a batch took another k_align instance than ext_geometry gives its longest read: %s" % res["tile_wrong"]
    res["stderr"] = err
    return res


# name: (option set, list, environment, counts that must be > 0, counts that must be 0)
CONFIGS = {
    "default": ("sr", "cases", {}, ("wave_prep", "wave_finish", "n_early", "n_slow", "solo_early", "solo_slow", "closed_form", "n_jobs"), ("reruns",)),
    "lanes_only": ("sr", "cases", {"AL_PREP_HEAVY": "0", "AL_FIN_HEAVY": "0"}, ("closed_form", "n_early", "n_slow"), ("wave_prep", "wave_finish")),
    "waves_always": ("sr", "cases", {"AL_PREP_HEAVY": "2", "AL_FIN_HEAVY": "2"}, ("wave_prep", "wave_finish", "n_early", "n_slow"), ()),
    "all_monolithic": ("sr", "cases", {"AL_DBG": str(1 << 26)}, ("mono_all",), FAST),
    "no_closed_form": ("sr", "cases", {"AL_DBG": str(-(1 << 31))}, ("n_jobs", "wave_prep"), ("closed_form",)),
    "no_hit_ordering": ("sr", "cases", {"AL_DBG": str(1 << 18)}, ("n_jobs",), ("wave_prep", "wave_finish")),
    "early_exit_off": ("sr", "cases", {"AL_DP_EXIT": "0"}, ("n_jobs", "closed_form"), ()),
    "two_cell_dp_off": ("sr", "cases", {"AL_DP_PK": "0"}, ("n_jobs", "closed_form"), ()),
    "scrubbed_0": ("sr", "cases", {"AL_TEST_SCRUB": "0"}, ("n_jobs",), ()),
    "scrubbed_255": ("sr", "cases", {"AL_TEST_SCRUB": "255"}, ("n_jobs",), ()),
    "guarded": ("sr", "cases", {"AL_TEST_GUARD": "1"}, ("n_jobs",), ()),
    "arena_overflow": ("sr", "arena", {}, ("reruns", "wave_prep"), ("mono_all",)),
    "long_mode": ("sr", "long", {}, ("long_mode", "mono_all"), FAST),
}
for _name in K.OPTION_SETS:
    if _name != "sr":
        # (no closed form either with zdrop below b + max(q + e, q2 + e2) = 33: the kernel's own rule, d_ext_prep_frag's diag_ok)
        _none = _name in ("no_closed_form", "zdrop30")
        CONFIGS["set_" + _name] = (_name, "cases", {}, ("n_jobs",) + (() if _none else ("closed_form",)), ("closed_form",) if _none else ())


@pytest.mark.parametrize("name", list(CONFIGS))
def test_extension_stage_equals_reference(name):
    optname, which, env, reached, unused = CONFIGS[name]
    res = run_child(optname, which, env)
    c = res["counts"]
    for k in reached:
        assert c[k] > 0, "the configuration did not reach what it is named for (%s): %s" % (k, c)
    for k in unused:
        assert c[k] == 0, "%s should be 0 here: %s" % (k, c)
    if which == "cases":                                                      # every LDS tile by its batch, and k_align_long for the batch one base beyond the largest
        assert set(res["tiles"]) == {"336", "512", "1024", "0"}, res["tiles"]
        assert c["long_mode"] == res["tiles"]["0"] == 1 and c["mono_all"] == (res["batches"] if name == "all_monolithic" else 1)
    if which == "long":
        assert set(res["tiles"]) == {"0"}
    if name == "guarded":
        assert "GUARD" not in res["stderr"], res["stderr"][-2000:]

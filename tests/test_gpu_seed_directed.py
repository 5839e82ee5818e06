"""The sketch, seed-lookup and anchor kernels (K1 ... K3) against the reference, read by read and fragment by fragment, on the directed cases of
tests/seed_cases.py: every read's minimizers against mm_sketch; of every fragment, in the first pass and in the re-chain pass, n_a, rep_len, the list
count and the anchors (x and y bit for bit, in the reference's order) against collect_seed_hits_heap; the per-fragment flag word against the ties in
the reference's anchors and the sort kernels' tables; and the counts that say which sort kernel got how many fragments against what the reference's
anchor counts and the switches in force imply.  tests/test_seed_oracle_cpu.py proves from the reference alone that the cases hold what they name.

The fragments go through al_dbg_seed -- what a batch run launches of a pass up to the chaining: k_sketch, k_seed, the size classes, the sort kernels,
the run merge or the device radix sort on their stream, the heap merges on theirs, the merges made ahead of the re-chain pass -- each configuration
in a fresh process (tests/helpers/seed_directed_child.py): the environment switches are read once per process.

Not reached: rank_bits < 0 (the flag-everything branch above the register tiles) needs a contig-id x position range above 2^46.  A fragment has one
or two segments: al_batch_upload accepts no more.  The tap gives every heap-merge launch (k_anchor_heap_lanes<2|1>,
k_anchor_heap<0|48|96>, k_anchor_heap_wave) a counter word of its own; each must equal the flagged fragments whose list and anchor counts put them there.

Measured on an MI355X: see TIMES below."""
import json
import os
import subprocess
import sys

import pytest

import seed_cases as K

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "seed_directed_child.py")
SWITCHES = ("AL_TEST_RUN", "AL_TEST_SORT_BLK", "AL_TEST_SORT_BIG", "AL_TEST_BIG_CHUNK", "AL_BIG_MERGE", "AL_HEAP_OLD", "AL_TEST_HEAP_WAVE", "AL_SPEC_MIN", "AL_SPEC_MERGE", "AL_TEST_POISON",
            "AL_TEST_POISON_ONLY", "AL_TEST_GUARD", "AL_DBG", "AL_DBG2", "AL_TEST_TILE_ALL", "AL_TRACE")
# A child's time limit: generating the cases and the reference's results takes 1 ... 2 s on a CPU, importing the package and building the host index
# 1 ... 3 s, the two passes on the GPU well under a second (TIMES); ten times that for a loaded machine.
LIMIT = 90
REGS = ("reg_2_1_128", "reg_4_1_256", "reg_8_1_512", "reg_16_1_512", "reg_8_4_1024", "reg_16_4_1024", "reg_16_8_1024")


def run_child(args, env):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env)
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable, CHILD] + list(args), capture_output=True, env=e)
    err = r.stderr.decode()
    assert r.returncode == 0, "[%s, %s] exit status %d\n%s\n%s" % (args, env, r.returncode, r.stdout.decode()[-3000:], err[-3000:])
    res = json.loads(r.stdout.decode().strip().split("\n")[-1])
    assert res["n_mismatch"] == 0, "[%s, %s] %d differences\n%s" % (args, env, res["n_mismatch"], "\n".join(res["mismatches"]))
    assert res["compared"] == res["generated"] > 0                          # nothing skipped or filtered out after generation
    if "AL_TEST_GUARD" in env:
        assert "GUARD:" not in err, err[-3000:]
    return res, err


LANE_FORMS = ("heap_lanes1", "heap_lanes2")
OLD_FORMS = ("heap_wave", "heap_serial48", "heap_serial96")
SMALL_RUNS = {"AL_TEST_RUN": "64,16", "AL_TEST_SORT_BIG": "65"}
POISON = {"AL_TEST_POISON": "170", "AL_TEST_GUARD": "1"}
# name: (environment, counts that must be > 0 in the first pass / the re-chain pass, counts that must be 0 there)
CONFIGS = {
    "default": ({}, (("small", "merge_frags", "heap_lanes1", "heap_lanes2", "heap_serial0") + REGS,) * 2, (("sort1024", "radix_frags", "flag_all") + OLD_FORMS,) * 2),
    # (AL_TEST_SORT_BIG is raised to the block sorts' bound: the run merge takes the fragments from 1025 anchors on, in runs of 64 / 128 keys)
    "run_merge_small_runs": (SMALL_RUNS, (("small", "merge_frags") + REGS[:4],) * 2, (REGS[4:] + ("radix_frags",),) * 2),
    "run_merge_small_runs_128": ({"AL_TEST_RUN": "128,128", "AL_TEST_SORT_BIG": "65"}, (("small", "merge_frags") + REGS[:4],) * 2, (REGS[4:] + ("radix_frags",),) * 2),
    "run_merge_from_65": (dict(SMALL_RUNS, AL_TEST_SORT_BLK="65"), (("small", "merge_frags"),) * 2, (REGS + ("radix_frags",),) * 2),
    "block_sort_from_65": ({"AL_TEST_SORT_BLK": "65"}, (REGS[4:] + ("merge_frags",),) * 2, (REGS[:4],) * 2),
    "block_and_run": ({"AL_TEST_SORT_BLK": "65", "AL_TEST_SORT_BIG": "200"}, (("reg_8_4_1024", "merge_frags"),) * 2, (REGS[:4] + REGS[5:],) * 2),
    "device_radix": ({"AL_BIG_MERGE": "0"}, (("radix_frags",) + REGS,) * 2, (("merge_frags",),) * 2),
    "device_radix_chunks": ({"AL_BIG_MERGE": "0", "AL_TEST_BIG_CHUNK": "3"}, (("radix_frags",),) * 2, (("merge_frags",),) * 2),
    "run_merge_second_pass_only": ({"AL_BIG_MERGE": "2"}, (("radix_frags",), ("merge_frags",)), (("merge_frags",), ("radix_frags",))),
    # (the wavefront form starts at 8192 anchors in up to 128 lists unless AL_TEST_HEAP_WAVE lowers it: then it takes every flagged fragment of up to 128 lists)
    "serial_heaps": ({"AL_HEAP_OLD": "1"}, (("heap_serial48", "heap_serial96", "heap_serial0"),) * 2, (("spec_made",) + LANE_FORMS,) * 2),
    "serial_heaps_wavefront": ({"AL_HEAP_OLD": "1", "AL_TEST_HEAP_WAVE": "1"}, (("heap_wave", "heap_serial0"),) * 2, (("spec_made", "heap_serial48", "heap_serial96") + LANE_FORMS,) * 2),
    "merge_ahead_every_candidate": ({"AL_SPEC_MIN": "1"}, (("heap_merges",), ("spec_made", "spec_taken")), ((), ())),
    "no_merge_ahead": ({"AL_SPEC_MERGE": "0"}, (("heap_merges",),) * 2, (("spec_made",), ("spec_made", "spec_taken"))),
    "poisoned_guarded": (POISON, (("small", "merge_frags", "heap_merges") + REGS,) * 2, ((), ())),
    "poisoned_guarded_small_runs": (dict(SMALL_RUNS, **POISON), (("merge_frags",),) * 2, ((), ())),
}


def check_counts(res, reached, unused, tag):
    for p, ks, zs in (("pass1", reached[0], unused[0]), ("pass2", reached[1], unused[1])):
        c = res[p]["counts"]
        for k in ks:
            assert c[k] > 0, "%s: the configuration did not reach what it is named for (%s, %s): %s" % (tag, p, k, c)
        for k in zs:
            assert c[k] == 0, "%s: %s should be 0 in %s: %s" % (tag, k, p, c)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_seed_stage_equals_reference(name):
    env, reached, unused = CONFIGS[name]
    res, err = run_child(["c3"], env)
    assert res["compared2"] == res["generated2"] > 100 and res["reads_compared"] == res["reads"] > res["generated"]
    check_counts(res, reached, unused, name)
    for p in ("pass1", "pass2"):
        s = res[p]; c = s["counts"]
        assert c["compact"] == 1 and c["rid_bits"] == 2
        assert s["tied_1_63"] > 0 and s["tied_64_126"] > 0 and s["tied_over_126"] > 0 and s["flagged_untied"] > 0
        assert s["flag1"] == c["flagged"] and s["flag1"] + s["flag2"] >= s["tied_1_63"] + s["tied_64_126"] + s["tied_over_126"]   # (the list leaves out what a merge made ahead covers)
        assert c["heap_merges"] == s["flag1"]                                 # every fragment flagged for a heap kernel was merged by exactly one
        if "AL_HEAP_OLD" not in env:                                          # the serial form takes exactly the flagged fragments of more than 126 lists
            assert c["heap_serial0"] == s["flag1_over_126"] > 0 and c["heap_lanes1"] + c["heap_lanes2"] == s["flag1"] - s["flag1_over_126"]
        if name == "serial_heaps_wavefront":                                  # the wavefront form takes every flagged fragment of up to 128 lists
            assert c["heap_wave"] == s["flag1_to_128"] > 0 and c["heap_serial0"] == s["flag1"] - s["flag1_to_128"]
    if "small_runs" in name or name == "run_merge_from_65":
        for p in ("pass1", "pass2"):
            assert res[p]["counts"]["merge_frags"] >= 3 and res[p]["counts"]["merge_passes"] >= 3
    if name == "default":
        assert res["pass1"]["counts"]["merge_passes"] >= 3                    # the fragment of 40 000 anchors at the default run length
    if name == "device_radix_chunks":
        assert res["pass1"]["counts"]["radix_chunks"] > 1 and res["pass2"]["counts"]["radix_chunks"] > 1
    if name == "merge_ahead_every_candidate":
        assert res["pass2"]["flag2"] == res["pass2"]["counts"]["spec_taken"] > 0
    else:
        assert res["pass2"]["flag2"] == 0


OTHER = {"default": {}, "device_radix": {"AL_BIG_MERGE": "0"}, "serial_heaps": {"AL_HEAP_OLD": "1"}}


@pytest.mark.parametrize("cfg", list(OTHER))
@pytest.mark.parametrize("shape", [s for s in K.SHAPES if s != "c3"])
def test_seed_stage_on_other_index_shapes(shape, cfg):
    res, err = run_child([shape], OTHER[cfg])
    assert res["compared2"] == res["generated2"] > 0 and res["reads_compared"] == res["reads"]
    n = K.SHAPES[shape].n_contigs
    assert res["n_contigs"] == n
    for p in ("pass1", "pass2"):
        c = res[p]["counts"]
        assert c["heap_merges"] == res[p]["flag1"] > 0 and c["small"] > 0 and c["flag_all"] == 0
        if cfg == "serial_heaps":                                           # (the flagged fragment of the long lists has 16 000 anchors in 18 lists: the wavefront form's at its own bound)
            assert c["heap_serial48"] + c["heap_wave"] > 0 and c["heap_lanes1"] == c["heap_lanes2"] == 0
        else:
            assert c["heap_lanes1"] > 0 and c["heap_wave"] == c["heap_serial48"] == c["heap_serial96"] == 0
        if n <= 32768:                                                      # compact keys: the register sorts; nothing for k_anchor_sort<1024>
            assert c["compact"] == 1 and c["sort1024"] == 0
            if not K.SHAPES[shape].long_list:
                assert all(c[k] > 0 for k in REGS[:5])
        else:                                                               # rid_bits above 15: k_anchor_sort<1024> up to 1024 anchors, the device radix sort from 1025 on
            assert c["compact"] == 0 and c["rid_bits"] >= 16 and c["sort1024"] > 0 and all(c[k] == 0 for k in REGS) and c["radix_frags"] > 0 and c["merge_frags"] == 0
    if shape == "c32768":
        assert res["pass1"]["counts"]["rid_bits"] == 15
    if K.SHAPES[shape].long_list:
        assert res["pass2"]["anchors"] > 40000


@pytest.mark.parametrize("k,w", K.SKETCH_SETS)
def test_sketch_equals_reference(k, w):
    """d_sketch<11> at w = 11, d_sketch<0> at the other windows, d_sketch_wide from k = 26 and, at (25, 11), for the batch that holds a read of 8192 bases."""
    res, err = run_child(["sketch", str(k), str(w)], {"AL_TEST_GUARD": "1"})
    assert res["batches"][-4:] == [1, 63, 64, 65] and res["minimizers"] > 300
    assert res["longest"] == (8192 if (k, w) == (25, 11) else 250)
    # the form k_sketch's arguments select, batch by batch: 1 d_sketch<11>, 2 d_sketch<0>, 3 d_sketch_wide
    want = [3 if k > 25 or (k == 25 and has) else 1 if w == 11 else 2 for has in res["with_8192"]]
    assert res["sketch_forms"] == want, (res["sketch_forms"], want)
    if (k, w) == (25, 11):
        assert want[0] == 3 and want[1] == 1                                  # the same reads with and without the one of 8192 bases


# Seconds per test, measured once on an MI355X (a child process end to end); inside the c3 child: 0.25 generating, 0.27 host index, 0.29 the two passes
# with their copies back, 0.03 comparing; inside the c65537 child the two passes take 0.05.  All 44 tests: 31 s.
TIMES = {"c3, any configuration": 1.1, "another index shape": 0.6, "a sketch option set": 0.6}

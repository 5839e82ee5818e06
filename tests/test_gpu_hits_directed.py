"""The kernels of the stage between chaining and extension against the reference's mm_gen_regs, mm_set_parent, mm_select_sub(_multi), mm_seg_gen and
mm_set_mapq (oracle/_ref/libhitref.so), fragment by fragment, mate by mate and hit by hit, on the directed chain sets of tests/hits_cases.py: the hit
count, every hit's id, parent, score, score0, cnt, rid, qs, qe, rs, re, subsc, n_sub, hash, mlen, blen, its rev / sam_pri / seg_split / seg_id flags
(every other flag bit 0), its anchors, and in a map-only context its MAPQ.  Integer equality throughout.

The fragments go through al_dbg_regs -- the stage's own host code: the chain-count classes of k_regs_select, k_regs_heavy_classify and the five
k_regs_heavy tiles, k_regs_cap2, the parts of k_regs, k_map_only and k_map_only_wave -- each configuration in a fresh process
(tests/helpers/hits_directed_child.py): the environment switches are read once per process.  Measured on an MI355X: a configuration takes about 3 s of
wall time, of which the case list and the reference take 1.1 s and the stage's calls 0.1 to 0.9 s."""
import json
import os
import subprocess
import sys

import pytest

import hits_cases as K

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "hits_directed_child.py")
SWITCHES = ("AL_DBG", "AL_DBG2", "AL_REGS_SPLIT", "AL_TEST_SCRUB", "AL_TEST_GUARD", "AL_TEST_POISON", "AL_DBG_FRAG")
CLASSES = ("class64", "class256", "class1024", "class2048", "class4096", "class8192", "class_above")
TILES = ("heavy12", "heavy24", "heavy48", "heavy72", "heavy200")


def run_child(optname, mode, which, env):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env)
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, CHILD, optname, mode, which], capture_output=True, env=e)
    err = r.stderr.decode()
    assert r.returncode == 0, "[%s %s, %s] exit status %d\n%s\n%s" % (optname, mode, env, r.returncode, r.stdout.decode()[-3000:], err[-3000:])
    res = json.loads(r.stdout.decode().strip().split("\n")[-1])
    print("[%s %s %s %s] %.1f s (cases and reference %.1f s, the stage's calls %.1f s)" % (optname, mode, which, env, res["seconds"], res["seconds_cases"], res["seconds_stage"]))
    assert res["n_mismatch"] == 0, "[%s %s, %s] %d fragments differ\n%s" % (optname, mode, env, res["n_mismatch"], "\n".join(res["mismatches"]))
    assert res["compared"] == res["generated"] > 800                       # nothing skipped or filtered out after generation
    assert res["counts"]["log_miss"] == 0                                  # no logf argument outside the table
    return res


# name: (option set, align | map_only, all | serial, environment, what must have been reached, what must not).  f1, f2, f3: fragments the selection kernels
# gave up with 0xfffffff1 ... 3.  (f3, a parent looked up beyond the REGS_KCAP kept records, needs more than 96 kept hits of which at most 64 are
# primaries: only best_n = 150 has them; with best_n = 1 no fragment keeps enough hits or anchors for the largest k_regs_heavy tile.)
CONFIGS = {
    "default": ("sr", "align", "all", {}, CLASSES + TILES + ("f2", "done", "kept", "unset"), ("f1",)),
    "one_kernel_for_1024": ("sr", "align", "all", {"AL_REGS_SPLIT": "0"}, CLASSES + TILES + ("f2", "done"), ("f1",)),
    "all_serial": ("sr", "align", "serial", {"AL_DBG": str(1 << 19)}, ("unset",), CLASSES + TILES + ("f1", "f2", "f3", "done", "kept", "select_ran")),
    "no_one_chain_path": ("sr", "align", "all", {"AL_DBG": str(1 << 20)}, CLASSES + TILES + ("one_chain_pairs",), ("f1",)),
    "ties_to_the_serial_code": ("sr", "align", "all", {"AL_DBG": str(1 << 16 | 1 << 17)}, CLASSES + ("f1", "f2"), ()),
    "scrubbed_0": ("sr", "align", "all", {"AL_TEST_SCRUB": "0"}, CLASSES + TILES, ("f1",)),
    "scrubbed_255": ("sr", "align", "all", {"AL_TEST_SCRUB": "255"}, CLASSES + TILES, ("f1",)),
    "map_only": ("sr", "map_only", "all", {}, CLASSES + TILES + ("mates_light", "mates_wave", "map_only_wave"), ("f1",)),
}
for _name in K.OPTION_SETS:
    if _name != "sr":
        CONFIGS[_name] = (_name, "align", "all", {}, CLASSES + (TILES[:4] if _name == "best_n1" else TILES) + (("alias_f3",) if _name == "best_n150" else ()), ("f1",))
CONFIGS["best_n150_map_only"] = ("best_n150", "map_only", "all", {}, CLASSES + TILES + ("alias_f3", "map_only_wave"), ("f1",))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_hit_stage_equals_reference(name):
    optname, mode, which, env, reached, unused = CONFIGS[name]
    res = run_child(optname, mode, which, env)
    c = dict(res["counts"]); c.update(res["regs_n0"]); c.update({k: res[k] for k in ("alias_f3", "one_chain_pairs", "mates_light", "mates_wave")})
    for k in reached:
        assert c[k] > 0, "the configuration did not reach what it is named for (%s): %s" % (k, c)
    for k in unused:
        assert c[k] == 0, "%s should be 0 here: %s" % (k, c)
    fr = K.cases(optname)
    if which == "serial":
        assert res["generated"] == sum(1 for f in fr if len(f.u) <= K.SERIAL_MAX_CHAINS) and res["chains_max"] >= 2049
    else:
        assert res["generated"] == res["listed"] == len(fr) and res["chains_max"] == 16500
        assert res["log_n_first_batch"] >= 16500 > K.LOGTAB_N               # the logf table of the batch of 150-base pairs holds logf(n_sub + 1) of its 16 500-chain fragment
    if mode == "map_only":
        assert c["map_only_wave"] == c["mates_wave"]                       # k_map_only_wave took exactly the mates of more than MO_LIGHT hits

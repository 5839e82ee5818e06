"""The second chaining round (the equal-x fragments) beside the first round's tile kernel: on the side stream, in a scratch set of its own.

AL_CHAIN_OVL=0 and one physical stream keep the round where it was, on main after the first round: the baseline.  Under AL_TRACE the chain stage says
per pass where the round ran ("second round (...): N equal-x fragments chained beside | after the first round") and per round what it reached
("round beside | main (...): tile kernel on ... deferred segments in C lane classes, ... to compact, ... handed back", "round ...: chain order kernels
on N fragments").  Every configuration runs in a process of its own: the environment switches are read once per process."""
import functools
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CHILD = os.path.join(HERE, "helpers", "chain_directed_child.py")
BATCH_CHILD = os.path.join(HERE, "helpers", "tie_beside_child.py")
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
# what a caller's environment must not carry into a child
SWITCHES = ("AL_TEST_TILE_ALL", "AL_TEST_TILE_FB", "AL_TEST_POISON", "AL_TEST_POISON_ONLY", "AL_TEST_GUARD", "AL_CHAIN_COOP", "AL_DBG", "AL_DBG2", "AL_CHAIN_WAVE_MAX", "AL_ORDER_BLOCK",
            "AL_TEST_SEG_BIG", "AL_CHAIN_OVL", "AL_CHAIN_OVL2", "AL_TEST_SORT_BLK", "AL_TEST_SORT_BIG", "AL_STREAMS", "AL_STREAM_MAP", "AL_TRACE")
SECOND = re.compile(r"\[airlift\] trace: second round \(first pass (\d)\): (\d+) equal-x fragments chained (beside|after) the first round( \([^)]*\))?")
ROUND = re.compile(r"\[airlift\] trace: round (beside|main) \(first pass (\d)\): tile kernel on (\d+) items, (\d+) deferred segments in (\d+) lane classes, (\d+) fragments to compact, (\d+) handed back")
ORDER = re.compile(r"\[airlift\] trace: round (beside|main): chain order kernels on (\d+) fragments")

ENVS = {
    "default": {},
    "chain_ovl_0": {"AL_CHAIN_OVL": "0"},
    "streams_1": {"AL_STREAMS": "1"},
    "streams_2": {"AL_STREAMS": "2"},
    "streams_10": {"AL_STREAMS": "10"},
    "tile_all_poisoned_guarded": {"AL_TEST_TILE_ALL": "1", "AL_TEST_POISON": "170", "AL_TEST_GUARD": "1"},
    "both_rounds_hand_everything_back": {"AL_TEST_TILE_ALL": "1", "AL_TEST_TILE_FB": "1"},      # two chain_fallback virtual batches alive at once
    "eight_wavefront_segment_forms": {"AL_TEST_SEG_BIG": "64"},
    "deferred_a_lane_each": {"AL_CHAIN_COOP": "0"},
    "deferred_sixteen_lanes": {"AL_CHAIN_COOP": "1"},
}
AFTER = ("chain_ovl_0", "streams_1")


def _child(cmd, env):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env, AL_TRACE="1")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable] + cmd, capture_output=True, env=e)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, "[%s, %s] exit status %d\n%s\n%s" % (cmd[1:], env, r.returncode, r.stdout.decode()[-3000:], err[-3000:])
    return json.loads(r.stdout.decode().strip().split("\n")[-1]), err


@functools.lru_cache(maxsize=None)
def _sr(name):
    return _child([CHILD, "sr"], ENVS[name])


@pytest.mark.parametrize("name", list(ENVS))
def test_sr_cases_equal_reference_wherever_the_round_runs(name):
    res, err = _sr(name)
    assert res["n_mismatch"] == 0, "[%s] %d fragments differ from mm_chain_dp\n%s" % (name, res["n_mismatch"], "\n".join(res["mismatches"]))
    assert res["compared"] == res["generated"] > 1000
    assert res["counts"]["tie_round"] > 0
    assert "GUARD:" not in err, err[-3000:]
    lines = SECOND.findall(err)
    assert len(lines) == res["batches"]                                       # one line per pass (a batch of the child is one pass)
    assert sum(int(n) for _, n, _, _ in lines) == res["counts"]["tie_round"] == res["flagged"]
    where = {w for _, n, w, _ in lines}
    if name in AFTER:
        assert where == {"after"}, lines
        assert {why for _, _, _, why in lines} == {" (AL_CHAIN_OVL=0)" if name == "chain_ovl_0" else " (one stream)"}
    else:
        # beside, except in the batches outside the tile kernel's range (the one with qlen_sum 4096): no tile kernel to run beside
        assert "beside" in where and sum(int(n) for _, n, w, _ in lines if w == "beside") > 0, lines
        assert {why for _, _, w, why in lines if w == "after"} <= {" (no tile kernel to run beside)"}, lines
        assert sum(1 for _, _, w, _ in lines if w == "after") < len(lines) / 2


def test_the_same_work_is_only_placed_elsewhere():
    a, b = _sr("default")[0]["counts"], _sr("chain_ovl_0")[0]["counts"]
    assert set(a) == set(b)
    for k in a:
        assert a[k] == b[k], (k, a, b)


def _reached(err, tag, first_pass):
    """What the round `tag` of a pass reached, from its trace lines: (deferred lane classes, to compact, handed back, order-kernel fragments) per al_dbg_chain call."""
    tiles = [(int(c), int(cmp_), int(fb)) for t, fp, _, _, c, cmp_, fb in ROUND.findall(err) if t == tag and int(fp) == first_pass]
    orders = [int(n) for t, n in ORDER.findall(err) if t == tag]
    return tiles, orders


def test_both_rounds_reach_every_shared_structure():
    """One al_dbg_chain batch whose flagged and unflagged fragments are the same fragments (tests/helpers/tie_beside_child.py): each round defers segments of
    at least three lane classes, compacts, gets fragments handed back for more than one reason (a segment longer than the tile is one) and runs the chain-order
    kernels, at the same time in two scratch sets.  Twice in one process, once more in a second, and once after the first round: byte-equal results."""
    two, err = _child([BATCH_CHILD, "2"], {})
    one, _ = _child([BATCH_CHILD, "1"], {})
    base, err0 = _child([BATCH_CHILD, "1"], {"AL_CHAIN_OVL": "0"})
    assert 200 <= two["fragments"] <= 1000 and two["anchors_max"] <= 2000 and two["flagged"] * 2 == two["fragments"]
    assert [(w, int(n)) for _, n, w, _ in SECOND.findall(err)] == [("beside", two["flagged"])] * 2
    assert [(w, int(n)) for _, n, w, _ in SECOND.findall(err0)] == [("after", two["flagged"])]
    for tag, first_pass in (("beside", 0), ("main", 1)):                     # (the tap's first round is a first pass; every second round is chain_tiles with first == false)
        tiles, orders = _reached(err, tag, first_pass)
        assert len(tiles) == 2 and len(orders) == 2, (tag, tiles, orders)
        for (classes, n_cmp, n_fb), n_order in zip(tiles, orders):
            assert classes >= 3 and n_cmp > 0 and n_order > 0 and n_fb > n_order, (tag, tiles, orders)
    assert len(set(two["digests"] + one["digests"] + base["digests"])) == 1, (two["digests"], one["digests"], base["digests"])
    assert two["counts"][0] == two["counts"][1] == one["counts"][0] == base["counts"][0]


def _write_paired_set(d):
    """A few thousand pairs whose mates overlap (inserts around 200: equal-x anchors), most of them inside a high-copy element (the re-chain pass)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_synth as g
    ref = g.make_reference(seed=5, n_contigs=2, total_len=900_000, n_dups=4, family=(1500, 200, 0.0))   # copies above mid_occ = 1000
    r1, r2 = g.simulate_pairs(ref, 3000, 150, seed=9, ins_mean=200, ins_sd=25, ins_lo=150, ins_hi=400)
    g.write_fasta(os.path.join(d, "ref.fa"), ref)
    g.write_fastq(os.path.join(d, "r_1.fq"), r1); g.write_fastq(os.path.join(d, "r_2.fq"), r2)


def test_sam_identical_wherever_the_round_runs(tmp_path):
    d = str(tmp_path)
    _write_paired_set(d)
    out = {}
    for name in ("default", "chain_ovl_0", "streams_1"):
        e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        e.update(ENVS[name], AL_TRACE="1")
        r = subprocess.run(["timeout", "-k", "10", "240", CLI, "-ax", "sr", "ref.fa", "r_1.fq", "r_2.fq"], cwd=d, capture_output=True, env=e)
        err = r.stderr.decode(errors="replace")
        assert r.returncode == 0, err[-3000:]
        lines = SECOND.findall(err)
        m = re.findall(r"trace: counters.* rechain=(\d+)", err)
        assert m and all(int(x) > 0 for x in m), "the set is meant to exercise the re-chain pass: %s" % m
        first = [(int(n), w) for fp, n, w, _ in lines if fp == "1"]; second = [(int(n), w) for fp, n, w, _ in lines if fp == "0"]
        assert first and second and all(n > 0 for n, _ in first) and all(n > 0 for n, _ in second), lines   # both passes have equal-x fragments
        assert {w for _, w in first + second} == ({"after"} if name in AFTER else {"beside"}), lines
        out[name] = r.stdout
    assert out["default"].count(b"\n") > 6000
    assert out["default"] == out["chain_ovl_0"] == out["streams_1"], {k: hashlib.sha256(v).hexdigest() for k, v in out.items()}

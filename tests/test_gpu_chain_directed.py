"""The chain stage's kernels against the reference's mm_chain_dp, fragment by fragment and in order, on the directed anchor sets of
tests/chain_cases.py: n_u, every u (score and count) and every chain's anchors, found through uo.

The fragments go through al_dbg_chain -- the stage's size classes and ordering, the lane kernels, the tile kernel or the segment-wise kernels,
the second round of the flagged fragments, the fallback and the chain-order kernels, on caller-supplied anchors -- each configuration in a
fresh process (tests/helpers/chain_directed_child.py): the environment switches are read once per process."""
import json
import os
import subprocess
import sys

import pytest

import chain_cases as K

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "chain_directed_child.py")
SWITCHES = ("AL_TEST_TILE_ALL", "AL_TEST_TILE_FB", "AL_TEST_POISON", "AL_TEST_POISON_ONLY", "AL_TEST_GUARD", "AL_CHAIN_COOP", "AL_DBG", "AL_DBG2", "AL_CHAIN_WAVE_MAX", "AL_ORDER_BLOCK",
            "AL_TEST_SEG_BIG", "AL_CHAIN_OVL", "AL_CHAIN_OVL2", "AL_TEST_SORT_BLK", "AL_TEST_SORT_BIG")
TILE_ALL = {"AL_TEST_TILE_ALL": "1"}


def run_child(optname, env):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env)
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, CHILD, optname], capture_output=True, env=e)
    err = r.stderr.decode()
    assert r.returncode == 0, "[%s, %s] exit status %d\n%s\n%s" % (optname, env, r.returncode, r.stdout.decode()[-3000:], err[-3000:])
    res = json.loads(r.stdout.decode().strip().split("\n")[-1])
    assert res["n_mismatch"] == 0, "[%s, %s] %d fragments differ\n%s" % (optname, env, res["n_mismatch"], "\n".join(res["mismatches"]))
    assert res["compared"] == res["generated"] > 1000                       # nothing skipped or filtered out after generation
    assert res["tied_starts"] >= 50 and res["flagged"] > 0 and res["empty_between_kept"] > 0 and res["chains_max"] > 128
    return res, err


# name: (option set, environment, counts that must be > 0, counts that must be 0).  (legacy_frags is never 0: the batch with qlen_sum 4096 is
# outside the LDS forms under every configuration and takes the segment-wise kernels.)
CONFIGS = {
    "default": ("sr", {}, ("lane_lo", "wave_mid", "tile_items", "deferred", "compacted", "handed_back", "fallback_frags", "order_frags", "tie_round"), ()),
    "tile_all": ("sr", TILE_ALL, ("tile_items", "deferred", "compacted", "handed_back", "fallback_frags", "order_frags", "tie_round"), ("lane_mid", "wave_mid")),
    "tile_all_poisoned_guarded": ("sr", dict(TILE_ALL, AL_TEST_POISON="170", AL_TEST_GUARD="1"), ("tile_items", "deferred", "compacted", "handed_back"), ()),
    "tile_hands_everything_back": ("sr", dict(TILE_ALL, AL_TEST_TILE_FB="1"), ("tile_items", "handed_back", "fallback_frags"), ()),
    "deferred_sixteen_lanes": ("sr", dict(TILE_ALL, AL_CHAIN_COOP="1"), ("deferred", "deferred_coop"), ()),
    "deferred_a_lane_each": ("sr", dict(TILE_ALL, AL_CHAIN_COOP="0"), ("deferred",), ("deferred_coop",)),
    "segment_kernels": ("sr", {"AL_DBG": str(1 << 28)}, ("lane_lo", "legacy_frags", "wave_segs", "order_frags"), ("tile_items",)),
    "wavefront_kernel_everywhere": ("sr", {"AL_DBG": str(1 << 27)}, ("legacy_frags", "wave_segs"), ("lane_lo", "lane_mid", "wave_mid", "tile_items", "lds_ok_any")),
    "thin_class_never": ("sr", {"AL_CHAIN_WAVE_MAX": "0"}, ("lane_lo", "lane_mid", "tile_items"), ("wave_mid",)),
    "thin_class_always": ("sr", {"AL_CHAIN_WAVE_MAX": "100000000"}, ("lane_lo", "wave_mid", "tile_items"), ("lane_mid",)),
    "thin_class_never_segment_kernels": ("sr", {"AL_CHAIN_WAVE_MAX": "0", "AL_DBG": str(1 << 28)}, ("lane_mid", "legacy_frags"), ("wave_mid", "tile_items")),
    "order_block_65": ("sr", {"AL_ORDER_BLOCK": "65"}, ("order_frags",), ()),
    "order_block_never": ("sr", {"AL_ORDER_BLOCK": "100000"}, ("order_frags",), ()),
    "eight_wavefront_segment_forms": ("sr", {"AL_TEST_SEG_BIG": "64"}, ("seg_big", "fallback_frags"), ()),
    "eight_wavefront_segment_forms_everywhere": ("sr", {"AL_TEST_SEG_BIG": "64", "AL_DBG": str(1 << 28)}, ("seg_big", "legacy_frags"), ("tile_items",)),
}
# what the option sets select on their own: (lds_ok, tiles_ok) of the batches of up to 4095 bases
PATHS = {"bw500": (1, 1), "skip0": (1, 0), "skip5": (1, 0), "skip6": (1, 0), "skip7": (1, 1), "iter128": (1, 1), "iter127": (0, 0), "min_cnt1": (1, 0), "min_cnt3_sc40": (1, 1),
         "max_gap40000": (0, 0), "k15": (1, 1), "k28": (1, 1)}
for _name, (_lds, _tiles) in PATHS.items():
    for _tag, _env in (("", {}), ("_tile_all", TILE_ALL)):
        CONFIGS[_name + _tag] = (_name, _env, (("tile_items",) if _tiles else ("legacy_frags",)) + (("lane_lo",) if _lds and not (_tiles and _env) else ()),
                                 (() if _tiles else ("tile_items",)) + (() if _lds else ("lane_lo", "lds_ok_any")))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_chain_stage_equals_reference(name):
    optname, env, reached, unused = CONFIGS[name]
    assert set(K.OPTION_SETS) == set(PATHS) | {"sr"}
    res, err = run_child(optname, env)
    c = res["counts"]
    for k in reached:
        assert c[k] > 0, "the configuration did not reach what it is named for (%s): %s" % (k, c)
    for k in unused:
        assert c[k] == 0, "%s should be 0 here: %s" % (k, c)
    assert c["lds_ok"] == 0                                                   # the batch with qlen_sum 4096 leaves the LDS forms under every option set
    assert res["over_64_anchors"] > 0
    if "AL_TEST_GUARD" in env:
        assert "GUARD:" not in err, err[-3000:]
    # the chain-order kernels got exactly the fragments with tied starts among more than 64 chains; k_chain_order_t<16> takes those of at least
    # AL_ORDER_BLOCK chains, k_chain_order_t<1> the others (the reference's n_u decides which, as the kernels' own count does)
    n_order = res["order_block_frags"] + res["order_wave_frags"]
    if K.OPTION_SETS[optname].min_cnt >= 2:
        assert c["order_frags"] == n_order > 0, (c, res["order_block_frags"], res["order_wave_frags"])
    else:                                                                    # (a chain of one anchor leaves no room for the processing keys: chained whole by the wavefront kernel instead)
        assert c["order_frags"] == 0 and c["whole_wave"] == n_order > 0, (c, n_order)
    if name == "order_block_65":
        assert res["order_block_frags"] > 0 and res["order_wave_frags"] == 0
    if name == "order_block_never":
        assert res["order_block_frags"] == 0 and res["order_wave_frags"] > 0
    if name == "default":
        assert res["order_block_frags"] > 0 and res["order_wave_frags"] > 0
    if name == "tile_hands_everything_back":
        assert c["handed_back"] * 2 > c["tile_frags"]                         # (tile_frags counts the flagged fragments in both rounds; the first skips them)

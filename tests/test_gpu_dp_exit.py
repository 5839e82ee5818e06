"""-m gpu: the early exit of the two-cells-per-lane extension DP (al_dev_ksw2.h).  The SAM must be the reference's with
the exit on, byte-identical with AL_DP_EXIT=0 under z-drop, band, gap and end-bonus settings that move the exit rule's terms, and the
shadow mode (AL_DBG2 bit 5: the rule is evaluated, the full DP still runs) must find no job whose outputs differ from the exit row's."""
import json
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
SETS = ["g1_mt150pe", "g2_250pe", "g3_adversarial", "g6_repeats"]
SHADOW = re.compile(rb"DP exit shadow \(two-cells-per-lane jobs\): jobs (\d+), differing (\d+); rows needed (\d+) of (\d+)")


def _run(d, m, extra=(), env=None):
    cmd = [CLI, "-ax", "sr"] + list(extra) + (["-R", m["rg"]] if m.get("rg") else [])
    r = subprocess.run(cmd + [m["ref"]] + m["reads"], cwd=d, capture_output=True, env=dict(os.environ, **(env or {})), timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout, r.stderr


@pytest.mark.parametrize("name", SETS)
def test_exit_gives_the_reference_sam(golden_unpacked, name):
    d = golden_unpacked[name]
    m = json.load(open(os.path.join(d, "meta.json")))
    exp = open(os.path.join(d, "expected.sam"), "rb").read()
    assert _run(d, m)[0] == exp
    assert _run(d, m, env=dict(AL_DP_EXIT="0"))[0] == exp


@pytest.mark.parametrize("name", ["g1_mt150pe", "g3_adversarial", "g6_repeats"])
@pytest.mark.parametrize("extra", [("-z", "25"), ("-z", "30"), ("-r", "8", "-z", "40"), ("--end-bonus", "0"), ("--end-bonus", "60"),
                                   ("-O", "6,26", "-E", "2,1"), ("-B", "12")],
                         ids=["z25", "z30", "bw8z40", "eb0", "eb60", "gaps", "mis12"])
def test_exit_equals_full_dp(golden_unpacked, name, extra):
    """The exit must not move a CIGAR, a score or an end position under settings that change U, E2 or E3."""
    d = golden_unpacked[name]
    m = json.load(open(os.path.join(d, "meta.json")))
    a = _run(d, m, extra)[0]
    b = _run(d, m, extra, env=dict(AL_DP_EXIT="0"))[0]
    assert a.count(b"\n") > 0
    assert a == b


@pytest.mark.parametrize("name", ["g1_mt150pe", "g3_adversarial", "g6_repeats"])
@pytest.mark.parametrize("extra", [(), ("-z", "30"), ("--end-bonus", "0")], ids=["sr", "z30", "eb0"])
def test_shadow_mode_finds_no_difference(golden_unpacked, name, extra):
    d = golden_unpacked[name]
    m = json.load(open(os.path.join(d, "meta.json")))
    out, err = _run(d, m, extra, env=dict(AL_DBG2="32"))
    assert out == _run(d, m, extra, env=dict(AL_DP_EXIT="0"))[0]       # (shadow mode leaves the results valid)
    hits = SHADOW.findall(err)
    assert hits, err.decode()[-2000:]
    jobs = sum(int(h[0]) for h in hits)
    assert jobs > 0
    assert sum(int(h[1]) for h in hits) == 0
    assert sum(int(h[2]) for h in hits) <= sum(int(h[3]) for h in hits)

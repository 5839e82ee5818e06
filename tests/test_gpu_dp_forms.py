"""-m gpu: the two-cells-per-lane extension DP (al_dev_ksw2.h, the default from 8 target blocks up) against the one-cell form
(AL_DP_PK=0) on the golden sets: the SAM must be the reference's with either form, and the two forms must agree with each other
under a small z-drop (many extensions stop inside the band) and a narrow band (rows clipped on both sides)."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
SETS = ["g1_mt150pe", "g2_250pe", "g3_adversarial", "g6_repeats"]


def _run(d, m, extra=(), env=None):
    cmd = [CLI, "-ax", "sr"] + list(extra) + (["-R", m["rg"]] if m.get("rg") else [])
    r = subprocess.run(cmd + [m["ref"]] + m["reads"], cwd=d, capture_output=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout


@pytest.mark.parametrize("name", SETS)
def test_both_forms_give_the_reference_sam(golden_unpacked, name):
    d = golden_unpacked[name]
    m = json.load(open(os.path.join(d, "meta.json")))
    exp = open(os.path.join(d, "expected.sam"), "rb").read()
    assert _run(d, m) == exp
    assert _run(d, m, env=dict(AL_DP_PK="0")) == exp


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("extra", [("-z", "25"), ("-r", "20"), ("-r", "8", "-z", "40")], ids=["z25", "bw20", "bw8z40"])
def test_packed_form_equals_one_cell_form(golden_unpacked, name, extra):
    """z-dropped and band-clipped extensions: every CIGAR, score and end position the records carry must be the same from both forms."""
    d = golden_unpacked[name]
    m = json.load(open(os.path.join(d, "meta.json")))
    a = _run(d, m, extra)
    b = _run(d, m, extra, env=dict(AL_DP_PK="0"))
    assert a.count(b"\n") > 0
    assert a == b

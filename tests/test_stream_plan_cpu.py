"""The stream plan of a mapping context (airlift_amd/csrc/al_stream_plan.h: which physical stream each of the ten stream roles runs on, for 1 ... 10
streams) as a stand-alone host program under AddressSanitizer + UBSan: `make san-stream-plan` links tests/csrc/stream_plan_main.cpp, which includes
nothing but that header."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "airlift_amd", "csrc")
ROLES = ["main", "side", "aux0", "aux1", "aux2", "ovl0", "ovl1", "ovl2", "spec", "spec2"]


@pytest.fixture(scope="module")
def printed():
    r = subprocess.run(["make", "san-stream-plan"], cwd=CSRC, capture_output=True)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "san_stream_plan")], capture_output=True, env=env, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
    out = {"plan": {}, "apart": [], "count": {}, "parse": {}}
    for l in r.stdout.decode().splitlines():
        f = l.split()
        if f[0] == "roles":
            out["roles"] = int(f[1])
        elif f[0] == "plan":
            out["plan"][int(f[1])] = [int(x) for x in f[2:]]
        elif f[0] == "apart":
            out["apart"].append((int(f[1]), int(f[2])))
        elif f[0] == "parse":
            out["parse"][f[1]] = int(f[3])
        elif f[0] == "count":
            out["count"][(f[1], f[2])] = (int(f[4]), int(f[5]))
    return out


def test_ten_roles_and_a_plan_for_every_count(printed):
    assert printed["roles"] == len(ROLES)
    assert sorted(printed["plan"]) == list(range(1, 11))
    assert all(len(m) == len(ROLES) for m in printed["plan"].values())


@pytest.mark.parametrize("n", range(1, 11))
def test_every_entry_below_n_and_every_stream_used(printed, n):
    m = printed["plan"][n]
    assert all(0 <= x < n for x in m), m
    assert sorted(set(m)) == list(range(n)), m


@pytest.mark.parametrize("n", range(1, 11))
def test_main_is_stream_0_and_shares_with_nobody(printed, n):
    m = printed["plan"][n]
    assert m[0] == 0
    if n >= 2:
        assert all(x != 0 for x in m[1:]), m


def test_ten_streams_is_the_identity(printed):
    assert printed["plan"][10] == list(range(10))


def test_one_stream_is_everything_on_main(printed):
    assert printed["plan"][1] == [0] * 10


@pytest.mark.parametrize("n", range(4, 11))
def test_never_together_pairs_are_apart(printed, n):
    """The header's own table (the plan function asserts against it as well), from n = 4 -- the default of a HIP process -- upwards."""
    assert len(printed["apart"]) >= 4
    spec, spec2, ovl0 = ROLES.index("spec"), ROLES.index("spec2"), ROLES.index("ovl0")
    assert (ovl0, spec) in printed["apart"] and (ovl0, spec2) in printed["apart"]      # the host waits for ovl0 in mid-step
    m = printed["plan"][n]
    for a, b in printed["apart"]:
        assert 0 <= a < 10 and 0 <= b < 10 and a != b
        assert m[a] != m[b], (ROLES[a], ROLES[b], m)


def test_stream_count_rule(printed):
    """AL_STREAMS (1 ... 10) first, else min(10, GPU_MAX_HW_QUEUES) as found in the environment, else HIP's default of 4; the second number is
    the source (0 AL_STREAMS, 1 environment, 2 default).  Values that are no positive integer count as unset."""
    c = printed["count"]
    assert c[("-", "-")] == (4, 2)
    assert c[("-", "4")] == (4, 1)
    assert c[("-", "16")] == (10, 1)
    assert c[("-", "2")] == (2, 1)
    assert c[("-", "0")] == (4, 2) and c[("-", "x")] == (4, 2)
    assert c[("1", "16")] == (1, 0)
    assert c[("6", "-")] == (6, 0)
    assert c[("10", "4")] == (10, 0)
    assert c[("99", "-")] == (10, 0)
    assert c[("0", "8")] == (8, 1) and c[("-3", "-")] == (4, 2)


def test_explicit_map_is_checked(printed):
    """AL_STREAM_MAP (experiments): ten numbers, main alone on 0, every stream up to the largest in use; anything else is ignored (0)."""
    p = printed["parse"]
    assert p["0,1,2,3,1,1,2,2,3,3"] == 4 and p["0,0,0,0,0,0,0,0,0,0"] == 1 and p["0,1,2,3,4,5,6,7,8,9"] == 10
    for bad in ("0,1,2,3,1,1,2,2,3", "0,1,2,3,1,1,2,2,3,3,1", "0,1,2,4,1,1,2,2,4,4", "1,0,2,3,1,1,2,2,3,3", "0,0,2,1,1,1,2,2,1,1", "0,1,2,3,1,1,2,2,3,x", "0,1,2,3,1,1,2,2,3,12", "empty", "-"):
        assert p[bad] == 0, bad

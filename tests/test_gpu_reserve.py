"""The device memory reserve (airlift_amd/csrc/al_devmem.cpp, its free list al_range_pool.h) on a small input.  The command line asks for a
reserve only from 2e5 reads on, so here a fresh process (tests/helpers/reserve_child.py: one reserve per process, the environment is read
once) calls al_device_reserve itself -- 500 MB in chunks of 125 MB -- then builds the index of golden set g1 on the device and maps the set
through al_map_file_frag.  The SAM must be the golden file, ranges must have been served from the reserve, and the report line must be the one
bench.py parses.  The second case adds AL_TEST_POISON / AL_TEST_GUARD: ranges the reserve recycles come back dirty, and fenced."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "reserve_child.py")
SWITCHES = ("AL_TEST_POISON", "AL_TEST_POISON_ONLY", "AL_TEST_POISON_LOG", "AL_TEST_GUARD", "AL_POOL_CHUNK_GB", "AL_NO_RESERVE", "AL_HBM_MARGIN_MB", "AL_TIMING")
# bench.py's expression for the report line
REPORT = (r"device memory reserve: ([0-9.]+) of ([0-9.]+) GB obtained in (\d+) chunk\(s\) of [0-9.]+ GB by the background thread in ([0-9.]+) s.*?"
          r"peak in use ([0-9.]+) GB, (\d+) ranges served, (\d+) requests passed on")


@pytest.mark.parametrize("env", [{}, {"AL_TEST_POISON": "170", "AL_TEST_GUARD": "1"}], ids=["plain", "poisoned_guarded"])
def test_small_run_served_from_the_reserve(golden_unpacked, tmp_path, env):
    d = golden_unpacked["g1_mt150pe"]
    out = tmp_path / "o.sam"
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env)
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, CHILD, d, str(out)], capture_output=True, env=e)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, "exit status %d\n%s\n%s" % (r.returncode, r.stdout.decode(errors="replace")[-2000:], err[-3000:])
    res = json.loads(r.stdout.decode().strip().split("\n")[-1])
    assert res["rc_reserve"] == 0 and res["rc_map"] == 0, res
    assert out.read_bytes() == open(os.path.join(d, "expected.sam"), "rb").read()
    assert res["peak"] > 0
    m = re.search(REPORT, res["report"])
    assert m, res["report"]
    assert res["report"].startswith("[airlift] device memory reserve: ") and res["report"].endswith(" requests passed on to hipMalloc\n")
    assert int(m.group(6)) > 0, res["report"]                                # ranges served
    assert "GUARD:" not in err, err[-3000:]

"""The free list of the device memory reserve (airlift_amd/csrc/al_range_pool.h: chunks, best fit with the lowest address on ties, coalescing
that stops at chunk ends, whole-free chunks taken out) as a stand-alone host program under AddressSanitizer + UBSan: `make san-range-pool`
links tests/csrc/range_pool_main.cpp, which includes nothing but that header and works on made-up addresses.  The program checks the header's
invariants after every operation and stops at the first violation; its directed cases come first, then 20 000 random operations against a
page-owner model."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "airlift_amd", "csrc")


@pytest.fixture(scope="module")
def printed():
    r = subprocess.run(["make", "san-range-pool"], cwd=CSRC, capture_output=True)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "san_range_pool")], capture_output=True, env=env, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
    return r.stdout.decode()


def test_directed_cases_hold(printed):
    assert "directed ok\n" in printed


def test_random_operations_agree_with_the_model_and_reach_both_answers(printed):
    m = re.search(r"^random served (\d+) refused (\d+)$", printed, re.M)
    assert m, printed
    assert int(m.group(1)) >= 1000 and int(m.group(2)) >= 1000, printed     # neither branch of the allocation is idle


def test_the_header_stands_alone():
    """No HIP include and no lock: the header includes only the standard containers it uses."""
    text = open(os.path.join(CSRC, "al_range_pool.h")).read()
    inc = re.findall(r"^#include\s+[<\"]([^>\"]+)[>\"]", text, re.M)
    assert sorted(inc) == ["map", "stddef.h", "stdint.h", "utility", "vector"], inc

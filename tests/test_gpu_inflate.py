"""k_inflate (al_inflate.hip) against the host twin over the case list of inflate_cases.py: bytes and status of every member, the guard-fenced variant,
more members than the grid has wavefronts, and two runs of the same list."""
import random

import pytest

import inflate_cases as ic
from inflate_util import inflate_device, inflate_host

pytestmark = pytest.mark.gpu


def _valid():
    return b"".join(c.data for c in ic.valid_cases())


def _mixed():
    """every valid case, a bad member (one of every member-level defect, going round) behind every third of them"""
    bad = [c for c in ic.invalid_cases() if ic.is_member_level(c)]
    out, k = [], 0
    for i, c in enumerate(ic.valid_cases()):
        out.append(c.data)
        if i % 3 == 0:
            out.append(bad[k % len(bad)].data); k += 1
    assert k >= len(bad)
    return b"".join(out)


@pytest.fixture(scope="module")
def twin():
    return {"valid": inflate_host(_valid()), "mixed": inflate_host(_mixed())}


def test_every_valid_case_in_one_launch(twin):
    rc, out, st = inflate_device(_valid())
    assert rc == 0 and not any(st) and len(st) > 700
    assert out == b"".join(c.expect for c in ic.valid_cases())
    assert (rc, out, st) == twin["valid"]


def test_the_mixed_list_equals_the_twin(twin):
    got = inflate_device(_mixed())
    assert got[0] == 0 and sum(1 for s in got[2] if s) > 100
    assert got[2] == twin["mixed"][2]
    assert got[1] == twin["mixed"][1]


def test_every_invalid_case_alone_equals_the_twin():
    for c in ic.invalid_cases():
        got = inflate_device(c.data)
        assert (got[0], got[2]) == (c.chain, c.codes), c.name
        assert got == inflate_host(c.data), c.name


def test_the_guard_ranges_stay_untouched(twin):
    got = inflate_device(_mixed(), guard=True)
    assert got[0] == 0, "rc %d (-7: a guard range was written)" % got[0]
    assert got == twin["mixed"]


def test_more_members_than_wavefronts_and_two_runs_agree():
    rng = random.Random(5000)
    payloads = [rng.randbytes(rng.randrange(1, 40)) * rng.randrange(1, 4) for _ in range(5000)]
    data = b"".join(ic.member(ic.deflate_raw(p, 6), p) for p in payloads)
    a = inflate_device(data)
    assert a[0] == 0 and a[2] == [0] * 5000 and a[1] == b"".join(payloads)
    assert inflate_device(data) == a

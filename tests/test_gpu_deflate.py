"""-m gpu tests of the BGZF compressor's kernel (k_deflate, al_deflate.hip) through the device backend: for every case of deflate_cases.py the members
must be the bytes of the host twin (al_dev_deflate.h: one function of a block's bytes, evaluated on both sides), which tests/test_deflate_cpu.py checks
as BGZF; they are inflated here once more directly."""
import random

import pytest

from deflate_cases import BLOCK, cases, n_blocks
from deflate_util import EOF_BLOCK, deflate_device, deflate_host, is_stored, members, stream_device, stream_device_resident

pytestmark = pytest.mark.gpu
CASES = cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_equals_host_twin(case):
    name, data, stored = case
    z, ns = deflate_device(data)
    ms = members(z)
    assert b"".join(r for _, r in ms) == data and len(ms) == n_blocks(len(data))
    assert ns == sum(is_stored(m) for m, _ in ms)
    if stored is not None:
        assert ns == stored
    h, hs = deflate_host(data)
    assert (len(z), ns) == (len(h), hs)
    assert z == h


def test_kernel_level_0_stores():
    data = random.Random(9).randbytes(1000) + bytes(2 * BLOCK)
    z, ns = deflate_device(data, level=0)
    assert ns == 3 and z == deflate_host(data, level=0)[0] and b"".join(r for _, r in members(z)) == data


def test_kernel_twice_the_same_bytes():
    data = b"".join(c[1] for c in CASES if c[0] in ("planted", "records_like", "window_edge_+0", "acgt_65281"))
    assert len(data) > 4 * BLOCK
    assert deflate_device(data) == deflate_device(data)


def test_more_blocks_than_workgroups():
    """600 short blocks' worth of bytes: every workgroup of the persistent grid takes several blocks, each from its own HBM scratch and LDS state"""
    rng = random.Random(4)
    unit = bytes(rng.choices(b"ACGTN", k=3000)) + rng.randbytes(300)
    data = (unit * (600 * BLOCK // len(unit) + 1))[:600 * BLOCK - 17]
    z, ns = deflate_device(data)
    assert (z, ns) == deflate_host(data)


@pytest.fixture(scope="module")
def stream():
    data = b"".join(c[1] for c in CASES if c[0] in ("records_like", "acgt_2_blocks", "random_65279", "planted", "zeros_195841", "period_7"))
    assert len(data) > 9 * BLOCK
    return data, stream_device(data, 0)


@pytest.mark.parametrize("piece", [1, BLOCK - 1, 100000])
def test_stream_cut_into_calls_gives_the_same_file(stream, piece):
    """AlBgzf's write path with the device backend (a flush every three blocks): however the bytes arrive, the file is the members of the stream's
    0xff00 grid and the EOF block"""
    data, whole = stream
    assert stream_device(data, piece) == whole
    assert whole == deflate_host(data)[0] + EOF_BLOCK


@pytest.mark.parametrize("mix", [False, True], ids=["device_only", "host_and_device_calls"])
@pytest.mark.parametrize("piece", [BLOCK - 1, BLOCK + 1, 100000, 3 * BLOCK + 17])
def test_device_resident_calls_give_the_host_held_file(stream, piece, mix):
    """the --bam fast path: a call's bytes lie in device memory and are compressed there; the first block of a call is gathered from the carry of the call
    before (in the seam buffer) and the call's head -- 1, 0xfeff and other numbers of carried bytes come up with these pieces -- and the members leave in
    64 KB pieces.  The file must be the one the host-held path writes."""
    data, whole = stream
    assert stream_device_resident(data, piece, mix) == whole


def test_device_resident_level_0_and_one_large_call(stream):
    data, whole = stream
    assert stream_device_resident(data, 0, ring=1 << 20) == whole
    z = stream_device_resident(data, 70000, level=0)
    assert z == stream_device(data, 0, level=0) and all(is_stored(m) for m, _ in members(z)[:-1])

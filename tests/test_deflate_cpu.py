"""CPU tests of the BGZF compressor of --gpu-deflate through its host twin (al_deflate_block_host, al_dev_deflate.h): the function the kernel computes,
evaluated serially.  The members must be BGZF blocks any inflater takes; tests/test_gpu_deflate.py then asks the kernel for the same bytes."""
import gzip
import os
import random
import subprocess

import pytest

from airlift_amd import capi
from deflate_cases import BLOCK, cases, n_blocks, planted
from deflate_util import deflate_host, is_stored, members

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
CASES = cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_twin_writes_bgzf_blocks(case):
    name, data, stored = case
    z, ns = deflate_host(data)
    ms = members(z)                                               # BC, BSIZE, CRC32, ISIZE of every member
    assert len(ms) == n_blocks(len(data))
    assert [len(r) for _, r in ms] == [BLOCK] * (len(ms) - 1) + [len(data) - BLOCK * (len(ms) - 1)] * (1 if ms else 0)
    assert b"".join(r for _, r in ms) == data
    if data:
        assert gzip.decompress(z) == data                         # (Python's gzip checks CRC32 and ISIZE once more)
    assert ns == sum(is_stored(m) for m, _ in ms)
    for m, r in ms:
        assert len(m) <= len(r) + 31
    if stored is not None:
        assert ns == stored, (name, ns, stored)


def test_level_0_stores_every_block():
    data = bytes(3 * BLOCK + 5)
    z, ns = deflate_host(data, level=0)
    ms = members(z)
    assert ns == 4 and all(is_stored(m) and len(m) == len(r) + 31 for m, r in ms) and b"".join(r for _, r in ms) == data


def test_random_bytes_come_back_stored_within_n_plus_31():
    data = random.Random(5).randbytes(2 * BLOCK)
    z, ns = deflate_host(data)
    assert ns == 2 and len(z) == len(data) + 2 * 31


def test_planted_matches_are_used():
    """every planted copy (lengths 3..258 at the first and last distance of every distance code) is bounded by a byte that ends it: the buffer must
    come out smaller than the same buffer with fresh random bytes in place of the copies"""
    a, _ = deflate_host(planted())
    b, _ = deflate_host(planted(fresh=True))
    assert len(planted()) == len(planted(fresh=True))
    assert len(a) < len(b) - 20000, (len(a), len(b))


def test_four_letters_compress_below_half():
    """random letters of a 4-letter alphabet carry 2 bits each; the greedy parse takes the chance 4-byte repeats too, which cost more than they save, so the
    bound is not the entropy's 0.25 but what any coding of four letters with whole bits guarantees with room to spare: below half, and not stored"""
    data = [c for c in CASES if c[0] == "acgt_2_blocks"][0][1]
    z, ns = deflate_host(data)
    assert ns == 0 and len(z) < len(data) // 2


def test_every_literal_and_every_length_symbol_in_one_block():
    """all_286_symbols, by the host twin's own token histogram: all 256 literals, the end-of-block symbol and the length symbols 258..285; symbol 257
    (length 3) is below the function's minimum match and must not occur"""
    import ctypes as C
    from deflate_cases import all_symbols
    data = all_symbols()
    hist = (C.c_uint32 * 316)()
    assert capi.load().al_dbg_deflate_hist(data, len(data), 5, hist) == 0
    assert all(hist[s] > 0 for s in range(256)) and hist[256] == 1
    assert hist[257] == 0
    assert [s for s in range(258, 286) if hist[s] == 0] == []
    assert sum(hist[258:286]) == sum(hist[286:316]) >= 255


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_selftest_crc_join_and_code_lengths(seed):
    """al_dbg_deflate_selftest: the CRC join against zlib's crc32 on random splits (zero-length parts among them); the code-length builder on adversarial
    histograms: Kraft sum <= 1, and = 1 from two used symbols on, no length above 15, zero frequency <=> zero length, cost <= the fixed code's, prefix-free codes"""
    assert capi.load().al_dbg_deflate_selftest(seed) == 0


REFUSED = [(["--gpu-deflate"], b"--bam or --sorted-bam"),
           (["--gpu-deflate", "--paf"], b"--bam or --sorted-bam"),
           (["--bam", "--gpu-deflate", "--devices", "0,0"], b"--devices"),
           (["--sorted-bam", "--gpu-deflate", "--devices", "0-1"], b"--devices"),
           (["--bam", "--gpu-deflate", "--world", "2", "--rank", "0", "-o", "x.bam"], b"--world"),
           (["--bam", "--gpu-deflate", "--ranked"], b"--ranked")]


@pytest.mark.parametrize("args,why", REFUSED, ids=[" ".join(a) for a, _ in REFUSED])
def test_cli_refuses_gpu_deflate_before_any_device_is_opened(args, why, tmp_path):
    ref = tmp_path / "ref.fa"; ref.write_text(">r\nACGTACGTAGCTAGCTAGCATCGATCGATCAGCTAGCTAGCATCGACTAGCTAGCTAC\n")
    fq = tmp_path / "r.fq"; fq.write_text("@a\nACGTACGTAGCTAGCTAGCA\n+\nIIIIIIIIIIIIIIIIIIII\n")
    env = dict(os.environ, RANK="0", WORLD_SIZE="2", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([CLI, "-ax", "sr"] + args + [str(ref), str(fq)], cwd=tmp_path, capture_output=True, env=env)
    assert r.returncode == 1
    assert b"[ERROR] --gpu-deflate" in r.stderr and why in r.stderr, r.stderr
    assert r.stdout == b""

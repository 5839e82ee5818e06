"""The listing-and-take function of the stream driver's BGZF input (airlift_amd/csrc/al_bgzf_take.h) under AddressSanitizer + UBSan: `make san-bgzf-take`
links tests/csrc/bgzf_take_main.cpp, a stand-alone program of host code only.  It feeds the function a member stream cut into pieces of every size from
1 byte up to twice the largest member, through a heap window of exactly the size the driver gives it, and asserts against a single-piece run that every
member comes out once, in order, with the right in_off and out_off.  Nothing loaded into python is sanitized."""
import os
import random
import subprocess

import inflate_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "airlift_amd", "csrc")


def _stream():
    """members of very unequal size: empty ones (EOF blocks, also in the middle), a few bytes, stored, well and badly compressible, extra subfields"""
    rng = random.Random(1414)
    out, n = [], 0
    for k in range(60):
        kind = k % 6
        if kind == 0:
            out.append(ic.EOF_BLOCK)
        elif kind == 1:
            p = rng.randbytes(rng.randrange(1, 4)); out.append(ic.member(ic.deflate_raw(p, 6), p))
        elif kind == 2:
            p = rng.randbytes(rng.randrange(200, 1500)); out.append(ic.member(ic.deflate_raw(p, 0), p))
        elif kind == 3:
            p = bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(500, 9000))); out.append(ic.member(ic.deflate_raw(p, 6), p))
        elif kind == 4:
            p = b"@r\nACGT\n+\nIIII\n" * rng.randrange(1, 4000); out.append(ic.member(ic.deflate_raw(p, 9), p))
        else:
            p = rng.randbytes(rng.randrange(1, 700)); out.append(ic.member(ic.deflate_raw(p, 5), p, before=ic.subfield(b"XY", b"abc"), after=ic.subfield(b"ZZ", b"")))
        n += 1
    return b"".join(out), n


def test_take_over_every_piece_size_under_asan_and_ubsan(tmp_path):
    r = subprocess.run(["make", "san-bgzf-take"], cwd=CSRC, capture_output=True)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    data, n = _stream()
    f = tmp_path / "members.bgzf"; f.write_bytes(data)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "san_bgzf_take"), str(f)], capture_output=True, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
    line = r.stdout.decode().strip().split("\n")[-1]
    assert line.startswith("san_bgzf_take: %d members, " % n), line
    largest = int(line.split("largest ")[1].split()[0])
    assert largest >= 1500 and ("%d piece sizes" % (2 * largest)) in line, line


def test_a_broken_chain_and_a_cut_last_member_are_told(tmp_path):
    data, _ = _stream()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    prog = os.path.join(CSRC, "build", "san_bgzf_take")
    assert subprocess.run(["make", "san-bgzf-take"], cwd=CSRC, capture_output=True).returncode == 0
    for name, bad, word in (("cut", data[:-5], b"bytes left at the end"), ("broken", data[:28] + b"\x00" + data[29:], b"chain broken at 28")):
        f = tmp_path / name; f.write_bytes(bad)
        r = subprocess.run([prog, str(f)], capture_output=True, env=env)
        assert r.returncode == 1 and word in r.stderr, (name, r.stdout + r.stderr)

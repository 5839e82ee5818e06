"""The BGZF compressor's host twin under AddressSanitizer + UBSan: `make san-deflate` links tests/csrc/deflate_main.cpp, a stand-alone program of host code
only, which compresses every case of deflate_cases.py block by block from exactly sized heap buffers and inflates the result."""
import os
import subprocess

from deflate_cases import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "airlift_amd", "csrc")


def test_host_twin_under_asan_and_ubsan(tmp_path):
    r = subprocess.run(["make", "san-deflate"], cwd=CSRC, capture_output=True)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    files = []
    for name, data, _ in cases():
        if data:
            p = tmp_path / name; p.write_bytes(data); files.append(str(p))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for level in ("5", "0"):
        r = subprocess.run([os.path.join(CSRC, "build", "san_deflate"), level] + files, capture_output=True, env=env)
        assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
        assert b"san_deflate:" in r.stdout

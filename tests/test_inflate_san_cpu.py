"""The BGZF inflater's host twin under AddressSanitizer + UBSan: `make san-inflate` links tests/csrc/inflate_main.cpp, a stand-alone program of host code
only, which inflates every member of every case of inflate_cases.py, valid and invalid, from exactly sized heap buffers into exactly sized ones and
asserts that no loop ran longer than its caps allow.  Nothing loaded into python is sanitized."""
import os
import subprocess
import zlib

import inflate_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "airlift_amd", "csrc")


def test_host_twin_under_asan_and_ubsan(tmp_path):
    r = subprocess.run(["make", "san-inflate"], cwd=CSRC, capture_output=True)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    cases = ic.valid_cases() + ic.invalid_cases()
    files = []
    for i, c in enumerate(cases):
        p = tmp_path / ("c%04d" % i); p.write_bytes(c.data); files.append(str(p))
    lst = tmp_path / "list.txt"; lst.write_text("\n".join(files) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "san_inflate"), str(lst)], capture_output=True, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
    lines = r.stdout.decode().strip().split("\n")
    assert lines[-1].startswith("san_inflate: %d files" % len(cases)), lines[-1]
    for c, line in zip(cases, lines):
        f = dict(kv.split("=") for kv in line.split()[1:])
        assert int(f["chain"]) == c.chain and [int(x) for x in f["st"].split(",") if x] == c.codes, (c.name, line)
        if c.expect is not None:
            assert int(f["out"]) == len(c.expect) and int(f["crc"], 16) == zlib.crc32(c.expect), (c.name, line)

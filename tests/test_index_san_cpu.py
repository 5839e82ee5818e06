"""The index of `airlift-align bam-index` on the host under AddressSanitizer + UBSan: `make san-bai` links tests/csrc/index_main.cpp, a stand-alone program of host
code only -- the kernels' twin (al_dev_bai.h), the member table, the piece / carry loop and the file's assembly (al_bai.h) -- which generates the shapes of
index_cases.san_specs(), takes each through the twin's loop at many piece sizes and prints a digest of each index; the digests are held against the rules restated
in Python.  Nothing loaded into python is sanitized."""
import os
import subprocess

import index_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "airlift_amd", "csrc")


def test_index_host_code_under_asan_and_ubsan():
    r = subprocess.run(["make", "san-bai"], cwd=CSRC, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "san_bai")], capture_output=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
    out = r.stdout.decode().strip().split("\n")
    specs = ic.san_specs()
    assert out[-1] == "san_bai: %d shapes" % len(specs), out[-1]
    got = {l.split(" ", 1)[0]: l.split(" ", 1)[1] for l in out[:-1]}
    assert sorted(got) == sorted(specs)
    for name, spec in specs.items():
        recs = ic.from_spec(spec); blob = ic.stream(recs); mem, file_end = ic.san_members(len(blob))
        if name.startswith("refused"):
            try:
                ic.expected_bai(ic.REFS, recs, mem); raise AssertionError(name)
            except ic.Refused:
                assert got[name] == "refused=-2", (name, got[name])
            continue
        want = ic.expected_bai(ic.REFS, recs, mem)
        f = dict(x.split("=") for x in got[name].split())
        assert int(f["bytes"]) == len(want) and f["digest"] == "%016x" % ic.fnv(want), (name, got[name])
    err = r.stderr.decode()
    assert "'input': not in coordinate order at offset" in err and "ends beyond 2^29" in err and "ends beyond its contig's length" in err, err[-2000:]

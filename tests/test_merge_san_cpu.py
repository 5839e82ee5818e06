"""The merge of `airlift-align merge` on the host under AddressSanitizer + UBSan: `make san-merge` links tests/csrc/merge_main.cpp, a stand-alone program of host
code only -- the headers' merge, the kernels' twin (al_dev_merge.h), the window rule and the round loop (al_merge.h) -- which generates the windows, ties and
unsorted shapes of merge_cases.san_specs(), takes each through the twin's round loop at many window sizes and prints a digest of the merged records; the digests
are held against the rules restated in Python.  Nothing loaded into python is sanitized."""
import os
import subprocess

import lift_cases as lc
import merge_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "airlift_amd", "csrc")
T = 256          # (the twin has no tile; a small one keeps the sweep over the window sizes short)


def test_merge_host_code_under_asan_and_ubsan():
    r = subprocess.run(["make", "san-merge"], cwd=CSRC, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "san_merge"), str(T)], capture_output=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
    out = r.stdout.decode().strip().split("\n")
    specs = mc.san_specs(T)
    assert out[-1] == "san_merge: %d shapes" % len(specs), out[-1]
    got = {l.split(" ", 1)[0]: l.split(" ", 1)[1] for l in out[:-1]}
    assert sorted(got) == sorted(specs)
    n_multi = 0
    for name, spec in specs.items():
        inputs = mc.from_spec(spec)
        if name.startswith("unsorted"):
            assert any(mc.descends(i[2]) for i in inputs) and got[name] == "refused=-2", (name, got[name])
            continue
        e = mc.expected(inputs)
        f = dict(x.split("=") for x in got[name].split())
        assert int(f["records"]) == len(e) and f["digest"] == "%016x" % mc.fnv(b"".join(lc.rec_bytes(o) for _, _, o in e)), (name, got[name])
        n_multi += int(f["rounds"]) > 1
    assert n_multi >= 10
    err = r.stderr.decode()
    assert all("'input %d': not in coordinate order at offset" % i in err for i in (1, 2)), err[-2000:]      # (a refusal prints its message at every window size)

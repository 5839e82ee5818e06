"""The lift of `airlift-align lift` on the host under AddressSanitizer + UBSan: `make san-lift` links tests/csrc/lift_main.cpp, a stand-alone program of host
code only -- the block table's builder, the header's parser and writer, the kernels' twin (al_dev_lift.h) and the piece / carry loop (al_lift.h) -- which walks
every directed BAM of lift_cases.py, the window shapes and the malformed inputs at every piece size from 64 bytes up (every size to 256, then in steps of 1/16 to
the stream's length) and holds the counts against the rules restated in Python.  Nothing loaded into python is sanitized."""
import os
import subprocess

import lift_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "airlift_amd", "csrc")


def test_lift_host_code_under_asan_and_ubsan(tmp_path):
    r = subprocess.run(["make", "san-lift"], cwd=CSRC, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    chain = tmp_path / "directed.chain"; chain.write_text(lc.CHAIN)
    sets = [("d%d" % n, lc.directed(n)) for n in lc.SIZES] + sorted(lc.walk_sets(8192).items())
    lines, expect = [], []
    for name, recs in sets:
        p = tmp_path / (name + ".bin"); p.write_bytes(lc.bam_bytes(lc.HEADER, lc.REFS, recs))
        v = lc.lift_all(lc.CHAIN, lc.REFS, recs)[0]
        lines.append("%s %s" % (p, chain)); expect.append((name, "kept=%d unlifted=%d unmapped=%d" % (v.count(lc.KEPT), v.count(lc.UNLIFTED), v.count(lc.UNMAPPED))))
    for name, (blob, say) in sorted(lc.malformed().items()):
        p = tmp_path / (name + ".bin"); p.write_bytes(blob)
        lines.append("%s %s" % (p, chain)); expect.append((name, "refused=-2"))
    lst = tmp_path / "list.txt"; lst.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "san_lift"), str(lst)], capture_output=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
    out = r.stdout.decode().strip().split("\n")
    assert out[-1] == "san_lift: %d files" % len(lines), out[-1]
    for (name, want), line in zip(expect, out):
        f = line.split(" ", 2)[2]
        assert f.split(" ", 1)[1] == want, (name, line, want)
        assert int(f.split()[0].split("=")[1]) > 100 or name in ("d0", "d1"), (name, line)

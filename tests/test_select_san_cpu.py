"""The selector of --gpu-select on the host under AddressSanitizer + UBSan: `make san-select` links tests/csrc/select_main.cpp, a stand-alone program of host
code only -- the name table's builder, the kernels' twin (al_dev_select.h) and the piece / carry / hand-over loop (al_select.h) -- which walks every case
text of select_cases.py at every piece size from 64 bytes up (every size to 256, then in steps of 1/16 to the text's length; every size of a text of at most 4096 bytes)
and holds the result against the default reader's.  Nothing loaded into python is sanitized."""
import os
import subprocess

import select_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "airlift_amd", "csrc")


def test_selector_host_code_under_asan_and_ubsan(tmp_path):
    r = subprocess.run(["make", "san-select"], cwd=CSRC, capture_output=True)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    cases = sc.cases(); lines = []; expect = []
    for c in cases:
        for k, (text, names) in enumerate(zip(c.fq, (c.l1, c.l2))):
            if k == 1 and c.name in ("none", "all", "probe5000"):      # (the texts of "base" again: one file of each is enough)
                continue
            fq = tmp_path / ("%s_%d.fq" % (c.name, k + 1)); fq.write_bytes(text)
            nm = tmp_path / ("%s_%d.names" % (c.name, k + 1)); nm.write_bytes(b"".join(n + b"\n" for n in names))
            lines.append("%s %s" % (fq, nm)); expect.append((c.name, k, c.handed[k]))
    lst = tmp_path / "list.txt"; lst.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "san_select"), str(lst)], capture_output=True, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
    out = r.stdout.decode().strip().split("\n")
    assert out[-1] == "san_select: %d files" % len(lines), out[-1]
    for (name, k, handed), line in zip(expect, out):
        f = dict(kv.split("=") for kv in line.split()[2:])
        assert int(f["handed"]) == handed and int(f["sizes"]) > 100, (name, k, line)
        assert (int(f["handover"]) >= 0) == (handed > 0 or name in ("trailing_blank", "seq_plus") and k == 0), (name, k, line)

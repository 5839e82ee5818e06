"""chain-exact on the host under AddressSanitizer + UBSan: `make san-chainexact` links tests/csrc/chainexact_main.cpp, a stand-alone program of host code only
-- the chain file's parser, the table builder, the kernels' twin, pass 3 and the printing (al_dev_chainexact.h).  It runs every g12 golden case in both
modes and at a second --min-region, and the refused chain files; the text of every run is held against the script's recorded bytes or the plain
restatement.  Nothing loaded into python is sanitized."""
import os
import subprocess

import chainexact_cases as cx
from test_chain_exact_cpu import CHAIN_REFUSED, FA_NEW, FA_OLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "airlift_amd", "csrc")


def test_chainexact_host_code_under_asan_and_ubsan(tmp_path):
    r = subprocess.run(["make", "san-chainexact"], cwd=CSRC, capture_output=True)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    lines, expect = [], []
    for name, p, want in cx.golden():
        old, new, chain = (open(p[k]).read() for k in ("old", "new", "chain"))
        for mode, M in (("verify", 100), ("build", 100), ("build", 7)):
            lines.append("%s %s %d %s %s %s" % (name, mode, M, p["old"], p["new"], p["chain"]))
            text = want[mode] if M == 100 else cx.restate(mode, old, new, chain, M)
            expect.append(("== %s %s %d\n" % (name, mode, len(text))).encode() + text)
    (tmp_path / "old.fa").write_text(FA_OLD); (tmp_path / "new.fa").write_text(FA_NEW)
    for k, (text, bad, _) in enumerate(CHAIN_REFUSED):
        fn = tmp_path / ("bad%d.chain" % k); fn.write_text(text)
        lines.append("bad%d build 100 %s %s %s" % (k, tmp_path / "old.fa", tmp_path / "new.fa", fn)); expect.append(("== bad%d refused\n%s:%d: " % (k, fn, bad)).encode())
    lst = tmp_path / "list.txt"; lst.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "san_chainexact"), str(lst)], capture_output=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr).decode(errors="replace")[-3000:]
    tail = ("san_chainexact: %d cases\n" % len(lines)).encode()
    assert r.stdout.endswith(tail)
    out = r.stdout[:-len(tail)]
    for e in expect:                                                       # in order, one behind the other
        assert out.startswith(e), e.split(b"\n")[0]
        out = out[len(e):] if b" refused\n" not in e else out[out.index(b"\n", len(e)) + 1:]
    assert out == b""

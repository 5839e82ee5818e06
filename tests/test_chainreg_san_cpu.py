"""The chain file's region logic of chain-beds / tokens --chain on the host under AddressSanitizer + UBSan: `make san-chainreg` links
tests/csrc/chainreg_main.cpp, a stand-alone program of host code only -- the parser of the chain file and of the merged BED, the kernels' twin and the BED
formatter (al_dev_chainreg.h).  It runs the g11 golden files, every table of chainreg_cases.py written out as a chain file, and the malformed files; the BED
text of every run is held against the plain restatement, the golden files' also against the scripts' recorded bytes.  Nothing loaded into python is
sanitized."""
import os
import subprocess

import chainreg_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "airlift_amd", "csrc")


def test_chainreg_host_code_under_asan_and_ubsan(tmp_path):
    r = subprocess.run(["make", "san-chainreg"], cwd=CSRC, capture_output=True)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    lines, expect = [], []
    golden = {c[0]: c for c in cc.golden()}
    for name, t, R, E, M in cc.cases():
        chain = tmp_path / (name + ".chain"); merged = tmp_path / (name + ".merged.bed")
        chain.write_text(golden[name[4:]][1] if name.startswith("g11_") else cc.chain_text(t))
        merged.write_text("".join("%s\t%d\t%d\n" % m for m in M))
        for with_m in (True, False):
            lines.append("%s %d %d %s %s" % (name, R, E, chain, merged if with_m else "-"))
            want = [("gaps", cc.bed(cc.gaps(t, R, E), t.names)), ("constant", cc.bed(cc.constant(t), t.names))]
            if with_m:
                want.append(("retired", cc.bed(cc.retired(t, M, R), cc.retired_slots(t, M))))
            if name.startswith("g11_"):
                for kind, text in want:
                    assert text == golden[name[4:]][5][kind], (name, kind)
            expect += [("== %s %s %d\n" % (name, kind, text.count(b"\n"))).encode() + text for kind, text in want]
    ok = tmp_path / "ok.chain"; ok.write_text(cc.HDR + "100\n")
    for k, (text, bad) in enumerate(cc.MALFORMED):
        fn = tmp_path / ("bad%d.chain" % k); fn.write_text(text)
        lines.append("bad%d 100 5 %s -" % (k, fn)); expect.append(("== bad%d refused\n%s:%d: " % (k, fn, bad)).encode())
    for k, (text, bad) in enumerate(cc.MERGED_MALFORMED):
        fn = tmp_path / ("badm%d.bed" % k); fn.write_text(text)
        lines.append("badm%d 100 5 %s %s" % (k, ok, fn)); expect.append(("== badm%d refused\n%s:%d: " % (k, fn, bad)).encode())
    lst = tmp_path / "list.txt"; lst.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "san_chainreg"), str(lst)], capture_output=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr).decode(errors="replace")[-3000:]
    tail = ("san_chainreg: %d cases\n" % len(lines)).encode()
    assert r.stdout.endswith(tail)
    got = r.stdout[:-len(tail)].split(b"== ")[1:]
    assert len(got) == len(expect)
    for g, e in zip(got, expect):
        if b" refused\n" in e:
            assert (b"== " + g).startswith(e) and g.count(b"\n") == 2, e
        else:
            assert b"== " + g == e, e.split(b"\n")[0]

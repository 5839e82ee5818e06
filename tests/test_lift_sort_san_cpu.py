"""The order of `airlift-align lift --sorted` on the host under AddressSanitizer + UBSan: `make san-lift-sort` links tests/csrc/lift_sort_main.cpp, a stand-alone
program of host code only -- the twin's compaction, descent count and stable sort (al_lift.h) and the run store's add, chain, spill, merge and finish
(al_run_store.h) -- which takes every directed set of lift_sort_cases.py through the piece loop at five piece sizes and, at each, through a store with limits
from 1 byte (a spill with every piece) upwards and without one, and prints counts and the hash of the merged output, held here against the rules restated in
Python.  Nothing loaded into python is sanitized, and nothing is preloaded."""
import os
import subprocess

import lift_cases as lc
import lift_sort_cases as ls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "airlift_amd", "csrc")


def fnv(h, b):
    for x in b:
        h = ((h ^ x) * 0x100000001b3) & 0xffffffffffffffff
    return h


def test_lift_sort_host_code_under_asan_and_ubsan(tmp_path):
    r = subprocess.run(["make", "san-lift-sort"], cwd=CSRC, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    chains = {lc.CHAIN: tmp_path / "directed.chain", ls.BIG_CHAIN: tmp_path / "big.chain"}
    for text, p in chains.items():
        p.write_text(text)
    lines, expect = [], []
    for name, (chain_text, recs) in sorted(ls.self_check().items()):
        p = tmp_path / (name + ".bin"); p.write_bytes(lc.bam_bytes(lc.HEADER, lc.REFS, recs))
        t = ls.truth(chain_text, lc.REFS, recs); v = t["v"]
        h = fnv(fnv(0xcbf29ce484222325, t["packed"]), "".join(x + "\n" for x in t["rows"]).encode())
        lines.append("%s %s" % (p, chains[chain_text]))
        expect.append((name, "kept=%d unlifted=%d unmapped=%d descents=%d" % (v.count(lc.KEPT), v.count(lc.UNLIFTED), v.count(lc.UNMAPPED), t["descents"]), "fnv=%016x" % h, len(t["perm"])))
    lst = tmp_path / "list.txt"; lst.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", TMPDIR=str(tmp_path))
    r = subprocess.run([os.path.join(CSRC, "build", "san_lift_sort"), str(lst)], capture_output=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr).decode(errors="replace")[-3000:]
    out = r.stdout.decode().strip().split("\n")
    assert out[-1] == "san_lift_sort: %d files" % len(lines), out[-1]
    for (name, counts, h, n_kept), line in zip(expect, out):
        f = line.split(" ")
        assert f[2] == "combos=25" and " ".join(f[3:7]) == counts and f[8] == h, (name, line, counts, h)
        assert int(f[7].split("=")[1]) >= (3 if n_kept > 40 else 0), (name, line)          # (spills: at a limit of one byte every piece with a record spills)

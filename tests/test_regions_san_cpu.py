"""The region merge of tokens --regions-bed / --merged-bed on the host under AddressSanitizer + UBSan: `make san-regions` links tests/csrc/regions_main.cpp, a
stand-alone program of host code only -- the fold's twin, the contig ranks and the BED formatter (al_dev_regions.h).  It runs every case list of
regions_cases.py through the twin, appended 0 (all at once), 1, 7 and n intervals at a time with a fold after each append, per gap and merged across the gaps,
and the BED text of every run is held against the plain restatement (sort the tuples, one loop).  The three random lists of 70 000 intervals take
1 000 and 7 001 in place of 1 and 7: a fold per interval of a list that keeps 35 000 regions is hours of sorting.  Nothing loaded into python is sanitized."""
import os
import subprocess

import regions_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "airlift_amd", "csrc")


def test_region_merge_host_code_under_asan_and_ubsan(tmp_path):
    r = subprocess.run(["make", "san-regions"], cwd=CSRC, capture_output=True)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    cases = rc.cases(); lines = []; expect = []
    for name, v, names in cases:
        chunks = [0, 1, 7, len(v)] if len(v) < 10000 else [0, 1000, 7001, len(v)]
        lines.append("case %s %d %d %d %s" % (name, len(v), len(names), len(chunks), " ".join(map(str, chunks))))
        lines += [n.decode() for n in names] + ["%d %d %d %d" % t for t in v]
        want = {pg: rc.merge(v, names, pg) for pg in (True, False)}
        for ch in chunks:
            for pg in (True, False):
                expect.append(("== %s %d %d %d\n" % (name, ch, int(pg), len(want[pg]))).encode() + rc.bed(want[pg], names))
    lst = tmp_path / "list.txt"; lst.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "san_regions"), str(lst)], capture_output=True, env=env)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr).decode(errors="replace")[-3000:]
    tail = ("san_regions: %d cases\n" % len(cases)).encode()
    assert r.stdout.endswith(tail)
    got = r.stdout[:-len(tail)].split(b"== ")[1:]
    assert len(got) == len(expect)
    for g, e in zip(got, expect):
        assert b"== " + g == e, e.split(b"\n")[0]
    # what the cases are there for
    by = {name: (v, names) for name, v, names in cases}
    assert [x[2:] for x in rc.merge(*by["book_ended"])] == [(10, 30)] and len(rc.merge(*by["gap_of_one"])) == 2
    assert [x[2:] for x in rc.merge(*by["long_nested"])] == [(1000, 120000), (120001, 120010)]
    assert len(rc.merge(*by["two_groups_same_coords"])) == 2 and len(rc.merge(*by["two_groups_same_coords"], per_gap=False)) == 1
    assert rc.bed(rc.merge(*by["ranks_reverse"]), rc.NAMES).startswith(b"c10\t5\t6\nc2\t5\t6\ncA\t5\t6\n")
    for n in rc.SIZES:
        assert len(rc.merge(*by["own_%d" % n])) == n and len(rc.merge(*by["one_%d" % n])) == 1
    assert len(rc.merge(*by["boundaries"])) == len(rc.SIZES) + 1
    for s in (11, 12, 13):
        assert 0.4 < len(rc.merge(*by["random_%d" % s])) / 70000.0 < 0.6

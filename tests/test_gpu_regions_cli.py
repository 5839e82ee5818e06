"""-m gpu tests of `airlift-align tokens --regions-bed / --merged-bed`, end to end: the BED files against the restatement (regions_cases.py) over the SAM the
same run prints without the options -- for the golden g7_tokens that SAM is the reference build's --, batched, with halved batches, with secondary
alignments, and through the C-ABI."""
import ctypes as C
import json
import os
import random
import subprocess

import pytest

import regions_cases as rc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")


def _run(args, cwd, **env):
    r = subprocess.run([CLI] + args, cwd=str(cwd), capture_output=True, env=dict(os.environ, **{k: str(v) for k, v in env.items()}))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r


def _gap_names(path):
    return [l[l.index(b">") + 1:].split(b">")[0].split()[0] for l in open(path, "rb") if b">" in l]


def _both(tok, files, cwd, extra=(), **env):
    """(per-gap BED, merged BED, stderr) of a regions run"""
    a, b = os.path.join(str(cwd), "regions.bed"), os.path.join(str(cwd), "merged.bed")
    for f in (a, b):
        if os.path.exists(f):
            os.remove(f)
    r = _run(tok + list(extra) + ["--regions-bed", a, "--merged-bed", b] + files, cwd, **env)
    assert r.stdout == b""
    return open(a, "rb").read(), open(b, "rb").read(), r.stderr


def _expected(sam, gaps):
    v, names = rc.sam_intervals(sam, gaps)
    return rc.bed(rc.merge(v, names, True), names), rc.bed(rc.merge(v, names, False), names), v, names


def test_g7_tokens_regions_are_those_of_the_reference_builds_sam(golden_unpacked):
    d = golden_unpacked["g7_tokens"]
    m = json.load(open(os.path.join(d, "meta.json")))
    sam = open(os.path.join(d, "expected.sam"), "rb").read()
    tok = ["tokens", "--read-size", str(m["read_size"]), "--skip", str(m["skip"])]; files = [m["ref"], m["gaps"]]
    per_gap, merged, _ = _both(tok, files, d)
    want = b"".join(b"MT_human\t%d\t%d\n" % se for se in ((100, 795), (3000, 3247), (6000, 6100), (9000, 10498), (12000, 12100), (15000, 15331)))
    assert per_gap == want and merged == want
    exp = _expected(sam, _gap_names(os.path.join(d, m["gaps"])))
    assert (exp[0], exp[1]) == (want, want) and len(exp[2]) == 337
    # one of the two on stdout, nothing else there
    r = _run(tok + ["--merged-bed", "-"] + files, d)
    assert r.stdout == want
    r = _run(tok + ["--regions-bed", "-", "--MD", "--eqx", "-Y"] + files, d)
    assert r.stdout == want
    # and without the options the SAM of before
    assert _run(tok + files, d).stdout == sam


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """Three contigs whose name order (c10, c2, cA) is not their index order (c2, cA, c10); c2[3000:5000] is planted at c10[1000:3000].  Gaps: two overlapping
    windows of c2 that reach into the planted segment, and one of N only."""
    d = tmp_path_factory.mktemp("regions_planted")
    rnd = random.Random(20261019)
    seq = {n: "".join(rnd.choice("ACGT") for _ in range(l)) for n, l in (("c2", 12000), ("cA", 8000), ("c10", 9000))}
    seq["c10"] = seq["c10"][:1000] + seq["c2"][3000:5000] + seq["c10"][3000:]
    with open(d / "ref.fa", "w") as f:
        for n in ("c2", "cA", "c10"):
            f.write(">%s\n" % n + "".join(seq[n][i:i + 70] + "\n" for i in range(0, len(seq[n]), 70)))
    with open(d / "gaps.fa", "w") as f:
        for n, s in (("c2:2500-4500", seq["c2"][2500:4500]), ("c2:3800-6000", seq["c2"][3800:6000]), ("nothing", "N" * 1500)):
            f.write(">%s\n" % n + "".join(s[i:i + 60] + "\n" for i in range(0, len(s), 60)))
    tok = ["tokens", "--read-size", "100", "--skip", "20"]; files = ["ref.fa", "gaps.fa"]
    sam = _run(tok + files, d).stdout
    return dict(d=d, tok=tok, files=files, sam=sam, gaps=_gap_names(d / "gaps.fa"), bed=_both(tok, files, d))


def test_planted_set_per_gap_and_merged(planted):
    p = planted
    assert p["gaps"] == [b"c2:2500-4500", b"c2:3800-6000", b"nothing"]
    want_pg, want_all, v, names = _expected(p["sam"], p["gaps"])
    assert names == [b"c2", b"cA", b"c10"] and len(v) > 150
    assert p["bed"][0] == want_pg and p["bed"][1] == want_all
    # the gap of N maps nowhere: every one of its tokens is an unmapped record, none an interval
    assert not [x for x in v if x[0] == 2] and p["sam"].count(b"nothing_") == 70
    # the two gaps overlap on c2: their own lines per gap, one line merged
    pg = [l.split(b"\t") for l in want_pg.splitlines()]; al = [l.split(b"\t") for l in want_all.splitlines()]
    c2 = [(int(s), int(e)) for c, s, e in pg if c == b"c2"]
    assert any(a[0] < b[1] and b[0] < a[1] for i, a in enumerate(c2) for b in c2[i + 1:])
    assert want_pg != want_all and len(al) < len(pg)
    assert [(c, int(s)) for c, s, e in al] == sorted((c, int(s)) for c, s, e in al)          # contig names in byte order, then start


def test_planted_set_batched_halved_and_with_secondaries(planted):
    p = planted
    a = _both(p["tok"], p["files"], p["d"], extra=["-K", "2000"])
    b = _both(p["tok"], p["files"], p["d"], AL_TEST_NOMEM_ABOVE=11)
    assert a[:2] == p["bed"][:2] and b[:2] == p["bed"][:2]
    assert b"does not fit the device workspaces" in b[2] and _run(p["tok"] + ["-K", "2000"] + p["files"], p["d"]).stdout == p["sam"]
    sec = ["--secondary=yes"]
    sam2 = _run(p["tok"] + sec + p["files"], p["d"]).stdout
    want_pg, want_all, v, _ = _expected(sam2, p["gaps"])
    got = _both(p["tok"], p["files"], p["d"], extra=sec + ["-K", "2000"])
    assert got[:2] == (want_pg, want_all)
    # with the secondary hits the planted copy is there for certain: tokens cut from c2 also land on c10, and c10 sorts in front of c2
    assert len(v) > len(rc.sam_intervals(p["sam"], p["gaps"])[0]) and want_all.startswith(b"c10\t") and b"\nc2\t" in want_all
    assert want_pg.startswith(b"c10\t") and want_pg != p["bed"][0]


def test_capi_gives_the_clis_bytes(planted):
    import airlift_amd as A
    p = planted; d = p["d"]
    L = A.load()
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p; libc.fopen.argtypes = [C.c_char_p, C.c_char_p]; libc.fclose.argtypes = [C.c_void_p]
    idx = A.Index(fasta=str(d / "ref.fa"), on_device=0)
    try:
        gaps = str(d / "gaps.fa").encode()
        assert L.al_map_tokens_regions(idx.h, gaps, 100, 20, C.byref(idx.mo), 3, None, None, 0) != 0
        fa, fb = libc.fopen(str(d / "capi_r.bed").encode(), b"wb"), libc.fopen(str(d / "capi_m.bed").encode(), b"wb")
        rcode = L.al_map_tokens_regions(idx.h, gaps, 100, 20, C.byref(idx.mo), 3, fa, fb, 0)
        libc.fclose(fa); libc.fclose(fb)
        assert rcode == 0
        fa = libc.fopen(str(d / "capi_only.bed").encode(), b"wb")
        rcode = L.al_map_tokens_regions(idx.h, gaps, 100, 20, C.byref(idx.mo), 3, None, fa, 0)
        libc.fclose(fa)
        assert rcode == 0
    finally:
        idx.close()
    assert open(d / "capi_r.bed", "rb").read() == p["bed"][0] and open(d / "capi_m.bed", "rb").read() == p["bed"][1]
    assert open(d / "capi_only.bed", "rb").read() == p["bed"][1]

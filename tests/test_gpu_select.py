"""-m gpu tests of --gpu-select: k_fq_select / k_fq_gather against their host twin through the taps, extract-sequence --gpu-select against the default
extract-sequence (plain and BGZF input), and remap --gpu-select against remap, with the selector's device memory gone when the call returns."""
import ctypes as C
import json
import os
import subprocess

import pytest

import select_cases as sc
from test_extract_cpu import write_bam
from test_select_cpu import CASES, OUT, run, timing

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")


def _tap(L, fn, text, names, *dev):
    n_cap = text.count(b"\n") // 4 + 2
    blob = b"".join(n + b"\n" for n in names)
    flags = (C.c_uint32 * n_cap)(); desc = (C.c_uint32 * (3 * n_cap))(); arena = C.create_string_buffer(len(text) + 16)
    n_rec, first_bad = C.c_uint64(0), C.c_uint64(0); arena_n, n_sel = C.c_size_t(0), C.c_size_t(0)
    rc = fn(*dev, text, len(text), blob, len(blob), flags, n_cap, C.byref(n_rec), C.byref(first_bad), arena, len(text) + 16, C.byref(arena_n), desc, n_cap, C.byref(n_sel))
    assert rc == 0, rc
    return list(flags[:n_rec.value]), first_bad.value, list(desc[:3 * n_sel.value]), arena.raw[:arena_n.value]


TAP_TEXTS = [("%s_%d" % (c.name, k + 1), c.fq[k], (c.l1, c.l2)[k]) for c in CASES for k in (0, 1) if not (c.name in ("none", "all", "probe5000") and k == 1)]
TAP_TEXTS += [("n%d" % n,) + sc.tap_text(n) for n in (63, 64, 65, 255, 256, 257)]


@pytest.mark.parametrize("name,text,names", TAP_TEXTS, ids=[t[0] for t in TAP_TEXTS])
def test_the_kernels_equal_their_host_twin(name, text, names):
    from airlift_amd import capi
    L = capi.load()
    host = _tap(L, L.al_dbg_fq_select_host, text, names)
    dev = _tap(L, L.al_dbg_fq_select, text, names, 0)
    assert dev[1] == host[1]                     # first_bad
    assert dev[0] == host[0]                     # flags
    assert dev[2] == host[2] and dev[3] == host[3]
    if name[0] == "n" and name[1:].isdigit():
        assert host[1] == 2 ** 64 - 1 and len(host[0]) == int(name[1:]) and sum(host[0]) == int(name[1:]) // 3
    if name == "base_1":
        assert 30 < sum(host[0]) < len(host[0]) and len(host[2]) == 3 * sum(host[0])


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_select")
    out = {}
    for c in CASES:
        if c.name not in ("base", "multiline", "crlf", "fasta", "seq_at"):
            continue
        p = d / c.name; p.mkdir()
        fq = [str(p / "r1.fq"), str(p / "r2.fq")]; rows = str(p / "rows.bed")
        for f, t in zip(fq, c.fq):
            open(f, "wb").write(t)
        z = [str(p / "r1.fq.gz"), str(p / "r2.fq.gz")]
        for f, t in zip(z, c.fq):
            open(f, "wb").write(sc.bgzf(t, 700 if c.name != "base" else 0xff00))
        open(rows, "wb").write(sc.rows(c.l1, c.l2))
        r, exp = run(fq + [rows], p / "default")
        assert r.returncode == 0, r.stderr.decode()
        out[c.name] = dict(fq=fq, z=z, rows=rows, exp=exp, dir=p, case=c)
    return out


@pytest.mark.parametrize("piece", [1000, 4096])
@pytest.mark.parametrize("bgzf", [False, True])
@pytest.mark.parametrize("name", ["base", "multiline", "crlf", "fasta", "seq_at"])
def test_extract_sequence_on_the_device_equals_the_default(files, name, bgzf, piece):
    f = files[name]
    args = ["--gpu-select"] + (["--gpu-inflate"] if bgzf else []) + ["--select-piece", str(piece)] + (f["z"] if bgzf else f["fq"]) + [f["rows"]]
    r, got = run(args, f["dir"] / ("d%d_%d" % (piece, bgzf)), AL_TIMING=1, **({"AL_INFLATE_PIECE_KB": 4} if bgzf else {}))
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    assert got == f["exp"]
    t = timing(r.stderr)
    assert len(t) == 2 and all(x[0] == "k_fq_select" for x in t), r.stderr.decode()[-1500:]
    assert [x[5] for x in t] == list(f["case"].handed)
    if name != "fasta":
        assert all(x[3] > 0 for x in t)
    assert r.stderr.count(b"device bytes held at return: 0\n") == 2


@pytest.fixture(scope="module")
def remap_case(golden_unpacked, tmp_path_factory):
    """The inputs of test_gpu_remap.py: g1_mt150pe, a BAM of its golden alignments, the same BED."""
    d = golden_unpacked["g1_mt150pe"]
    m = json.load(open(os.path.join(d, "meta.json")))
    t = tmp_path_factory.mktemp("gpu_select_remap")
    refs, recs = [], []
    for line in open(os.path.join(d, m["sam"]) if "sam" in m else os.path.join(d, "expected.sam")):
        f = line.rstrip("\n").split("\t")
        if line.startswith("@SQ"):
            refs.append((f[1][3:], int(f[2][3:])))
        if line.startswith("@") or int(f[1]) & 0x900 or f[2] == "*":
            continue
        cig, n = [], ""
        for ch in (f[5] if f[5] != "*" else ""):
            if ch.isdigit():
                n += ch
            else:
                cig.append((int(n), ch)); n = ""
        recs.append(([r[0] for r in refs].index(f[2]), int(f[3]) - 1, int(f[4]), int(f[1]), cig, f[0], len(f[9])))
    recs.sort(key=lambda r: (r[0], r[1]))
    bam = str(t / "old.bam"); write_bam(bam, refs, recs)
    bed = str(t / "regions.bed"); ln = refs[0][1]
    open(bed, "w").write("".join("%s\t%d\t%d\n" % (refs[0][0], b, e) for b, e in ((200, 3000), (2500, 6000), (9000, ln - 100))))
    return dict(ref=os.path.join(d, m["ref"]), fq=[os.path.join(d, r) for r in m["reads"]], bam=bam, bed=bed, tmp=t)


def test_remap_writes_the_same_sam_files_and_leaves_no_device_memory(remap_case):
    c = remap_case; t = c["tmp"]; env = dict(os.environ, AL_PG_PLAIN="1", AL_TIMING="1")
    out = {}
    for name, extra in (("default", []), ("select", ["--gpu-select"]), ("both", ["--gpu-select", "--gpu-inflate"])):
        p, s = str(t / (name + "_p.sam")), str(t / (name + "_s.sam"))
        r = subprocess.run([CLI, "remap", "--noprune"] + extra + ["-o", p, "--singletons", s, c["ref"], c["bam"], c["bed"]] + c["fq"], capture_output=True, env=env)
        assert r.returncode == 0, r.stderr.decode()[-1500:]
        out[name] = (open(p, "rb").read(), open(s, "rb").read())
        if extra:
            tl = timing(r.stderr)
            assert len(tl) == 2 and all(x[0] == "k_fq_select" and x[3] > 0 and x[5] == 0 for x in tl), r.stderr.decode()[-2000:]
            assert r.stderr.count(b"device bytes held at return: 0\n") == 2
    assert out["select"] == out["default"] and out["both"] == out["default"] and out["default"][0].count(b"\n") > 500

"""-m gpu tests of `airlift-align chain-beds` and `tokens --chain`, end to end.  chain-beds on the device must write the bytes the reference's scripts
wrote for the g11 golden cases.  On the `planted` three-contig reference of test_gpu_tokens_bed.py (rebuilt here) with a chain file over it, `tokens --chain`
must give the SAM, --regions-bed and --merged-bed bytes of `tokens --gaps-bed` over the gaps file `chain-beds --host --gaps-out` wrote, --gaps-out that file,
and --retired-bed / --constant-bed what `chain-beds --host --merged-in <that merged.bed>` gives -- also in several batches and through the C-ABI."""
import ctypes as C
import os
import random
import subprocess

import pytest

import chainreg_cases as cc
import tokens_cases as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
GOLDEN = cc.golden()
R, S, E = 100, 20, 5
# slot order (cA, c2, c10) is neither index order (c2, cA, c10) nor name order (c10, c2, cA); c10's tSize is not its length; a gap inside the planted copy
# (c2[3000:5000] = c10[1000:3000]), an insertion, gaps within R + E of both ends of a contig, two chains on c10 without a blank line between them, a second chain on cA behind a bare stretch
CHAIN = """# planted
chain 1 cA 8000 + 100 7900 qA 8000 + 0 7000 1
900 200 0
3000 0 25
1500 300 10
400

chain 2 c2 12000 + 0 12000 q2 12000 + 0 11000 2
3200 400 0
5000 50 0
3270 80 0

chain 3 c10 9100 + 50 5090 q10 9000 + 0 5000 3
30 10 0
5000
chain 4 c10 9100 + 8000 9100 q10 9000 + 7000 8000 4
900 150 0
50

chain 5 cA 8000 + 7000 7400 qA 8000 + 6000 6400 5
400
"""
GAPS = b"cA\t895\t1304\ncA\t4095\t4304\ncA\t5595\t6104\nc2\t3095\t3704\nc2\t8495\t8754\nc2\t11815\t11999\nc10\t0\t194\nc10\t8795\t9099\n"


def _run(args, cwd, **env):
    r = subprocess.run([CLI] + args, cwd=str(cwd), capture_output=True, timeout=120, env=dict(os.environ, AL_PG_PLAIN="1", **{k: str(v) for k, v in env.items()}))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r


@pytest.mark.parametrize("case", GOLDEN, ids=[c[0] for c in GOLDEN])
def test_chain_beds_on_the_device_writes_the_scripts_bytes(case, tmp_path):
    name, _, _, r_, e_, want = case
    chain = os.path.join(cc.G11, name + ".chain"); merged = os.path.join(cc.G11, name + ".merged.bed")
    r = _run(["chain-beds", "--read-size", str(r_), "--max-errors", str(e_), "--gaps-out", "g.bed", "--constant-bed", "c.bed", "--merged-in", merged, "--retired-bed", "-", chain], tmp_path)
    assert r.stdout == want["retired"] and (tmp_path / "g.bed").read_bytes() == want["gaps"] and (tmp_path / "c.bed").read_bytes() == want["constant"]


def _write_fa(path, seqs):
    with open(path, "w") as f:
        for n, s in seqs:
            f.write(">%s\n" % n.decode() + "".join(s[i:i + 70] + "\n" for i in range(0, len(s), 70)))


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """The reference of test_gpu_tokens_bed.py's `planted` set, the chain file over it, the gaps file the host twin writes, and the three outputs of
    `tokens --gaps-bed` over that file with the retired / constant rows the host twin makes of its merged.bed: what every run below is held against."""
    d = tmp_path_factory.mktemp("chain_planted")
    rnd = random.Random(20261019)
    seq = {n: "".join(rnd.choice("ACGT") for _ in range(l)) for n, l in (("c2", 12000), ("cA", 8000), ("c10", 9000))}
    seq["c10"] = seq["c10"][:1000] + seq["c2"][3000:5000] + seq["c10"][3000:]
    seq["cA"] = seq["cA"][:2000] + "N" * 1500 + seq["cA"][3500:5000] + seq["cA"][5000:5300].lower() + "R" + seq["cA"][5301:5600].lower() + seq["cA"][5600:]
    seqs = [(n.encode(), seq[n]) for n in ("c2", "cA", "c10")]
    assert [(n, len(s)) for n, s in seqs] == tc.CONTIGS
    _write_fa(d / "ref.fa", seqs)
    (d / "x.chain").write_text(CHAIN)
    tok = ["tokens", "--read-size", str(R), "--skip", str(S)]
    _run(["chain-beds", "--host", "--read-size", str(R), "--max-errors", str(E), "--gaps-out", "gaps.bed", "x.chain"], d)
    assert (d / "gaps.bed").read_bytes() == GAPS
    sam = _run(tok + ["--gaps-bed", "gaps.bed", "ref.fa"], d).stdout
    _run(tok + ["--gaps-bed", "gaps.bed", "--regions-bed", "w_regions.bed", "--merged-bed", "w_merged.bed", "ref.fa"], d)
    _run(["chain-beds", "--host", "--read-size", str(R), "--merged-in", "w_merged.bed", "--retired-bed", "w_retired.bed", "--constant-bed", "w_constant.bed", "x.chain"], d)
    want = dict(sam=sam, gaps=GAPS, **{k: (d / ("w_%s.bed" % k)).read_bytes() for k in ("regions", "merged", "retired", "constant")})
    # 16 + 6 + 21 + 26 + 8 + 5 + 5 + 6 tokens of the eight rows (range(R, len, S) of the bases faidx prints for each): five batches of -K 2000
    toks = tc.tokens([n for _, _, _, n in tc.rows(GAPS, tc.CONTIGS)], R, S)
    assert len(toks) == 93 and len({l.split(b"\t")[0] for l in sam.split(b"\n") if l and not l.startswith(b"@")}) == 93
    # the retired step's slots are the merged contigs in the merged BED's order (c10, c2, cA: name order), not the chain's (cA, c2, c10); c2 is covered
    assert want["merged"].count(b"\n") >= 8 and want["constant"].count(b"\n") == 12
    assert want["retired"] == b"c10\t5190\t7899\ncA\t6500\t6899\ncA\t7500\t7999\n"
    assert b"c10\t1" in want["merged"]                                     # the gap inside c2's planted stretch also maps to its copy on c10
    return dict(d=d, tok=tok + ["--chain", "x.chain", "--max-errors", str(E)], want=want)


def _chain_run(p, sub, extra=()):
    """the SAM run and the regions run of `tokens --chain` into directory sub: dict of every output's bytes, and the two stderr texts"""
    d = p["d"] / sub; d.mkdir()
    s = _run(p["tok"] + list(extra) + ["--gaps-out", str(d / "gaps_sam.bed"), "ref.fa"], p["d"])
    outs = {k: str(d / (k + ".bed")) for k in ("regions", "merged", "retired", "constant", "gaps")}
    r = _run(p["tok"] + list(extra) + ["--regions-bed", outs["regions"], "--merged-bed", outs["merged"], "--retired-bed", outs["retired"], "--constant-bed", outs["constant"], "--gaps-out", outs["gaps"], "ref.fa"], p["d"])
    assert r.stdout == b"" and (d / "gaps_sam.bed").read_bytes() == p["want"]["gaps"]
    return dict(sam=s.stdout, **{k: open(v, "rb").read() for k, v in outs.items()}), s.stderr, r.stderr


def test_tokens_chain_gives_the_bytes_of_the_gaps_bed_run_and_of_the_host_twin(planted):
    got, e_sam, e_reg = _chain_run(planted, "plain")
    assert got == planted["want"]
    for e in (e_sam, e_reg):                                              # c10: tSize 9100, 9000 bases -- one notice, and tSize rules (the row c10 8795 9099)
        assert e.count(b"tSize differs") == 1 and b"'c10'" in e and b"9100" in e
    # the retired rows without --merged-bed; '-' for one of the outputs
    r = _run(planted["tok"] + ["--retired-bed", "-", "ref.fa"], planted["d"])
    assert r.stdout == planted["want"]["retired"]
    r = _run(planted["tok"] + ["--constant-bed", "-", "ref.fa"], planted["d"])
    assert r.stdout == planted["want"]["constant"]


def test_tokens_chain_in_several_batches(planted):
    got, _, _ = _chain_run(planted, "batched", extra=["-K", "2000"])      # 20 tokens per batch
    assert got == planted["want"]


def test_capi_gives_the_clis_bytes(planted):
    import airlift_amd as A
    p = planted; d = p["d"]
    L = A.load()
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p; libc.fopen.argtypes = [C.c_char_p, C.c_char_p]; libc.fclose.argtypes = [C.c_void_p]
    idx = A.Index(fasta=str(d / "ref.fa"), on_device=0)
    names = ("regions", "merged", "retired", "constant", "gaps")
    try:
        chain = str(d / "x.chain").encode()
        assert L.al_map_tokens_chain_regions(idx.h, chain, E, R, S, C.byref(idx.mo), 3, None, None, 0, None, None, None) == -1
        f = {k: libc.fopen(str(d / ("capi_%s.bed" % k)).encode(), b"wb") for k in names}
        rcode = L.al_map_tokens_chain_regions(idx.h, chain, E, R, S, C.byref(idx.mo), 3, f["regions"], f["merged"], 0, f["retired"], f["constant"], f["gaps"])
        for k in names:
            libc.fclose(f[k])
        assert rcode == 0
        fs, fg = libc.fopen(str(d / "capi.sam").encode(), b"wb"), libc.fopen(str(d / "capi_gaps2.bed").encode(), b"wb")
        rcode = L.al_map_tokens_chain_file(idx.h, chain, E, R, S, C.byref(idx.mo), 3, fs, None, 0, fg)
        libc.fclose(fs); libc.fclose(fg)
        assert rcode == 0
        fa = libc.fopen(str(d / "capi_dev_gaps.bed").encode(), b"wb")
        rcode = L.al_chain_beds(chain, R, E, None, fa, None, None, 0, 0)
        libc.fclose(fa)
        assert rcode == 0
    finally:
        idx.close()
    for k in names:
        assert open(d / ("capi_%s.bed" % k), "rb").read() == p["want"][k], k
    assert open(d / "capi_gaps2.bed", "rb").read() == p["want"]["gaps"] and open(d / "capi_dev_gaps.bed", "rb").read() == p["want"]["gaps"]
    sam = open(d / "capi.sam", "rb").read()
    strip = lambda s: b"\n".join(l for l in s.split(b"\n") if not l.startswith(b"@PG"))
    assert strip(sam) == strip(p["want"]["sam"])

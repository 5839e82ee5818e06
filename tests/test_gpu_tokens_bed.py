"""-m gpu tests of `airlift-align tokens --gaps-bed`, end to end: for a gaps BED the equivalent GAPS.fa is made by tokens_cases.gaps_fasta (what
`samtools faidx REF name:a-b` prints per row), and the SAM and both regions files of the BED run are held against those of `tokens REF GAPS.fa` byte for
byte -- batched, one token per batch, with halved batches, with secondary alignments and through the C-ABI -- and, for the golden g10_gaps_bed, against the
reference build's SAM and the restatement of the region merge over it."""
import ctypes as C
import json
import os
import random
import subprocess

import pytest

import regions_cases as rc
import tokens_cases as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")


def _run(args, cwd, **env):
    r = subprocess.run([CLI] + args, cwd=str(cwd), capture_output=True, env=dict(os.environ, **{k: str(v) for k, v in env.items()}))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r


def _all(tok, src, cwd, extra=(), **env):
    """(SAM, per-gap BED, merged BED, stderr of the SAM run, stderr of the regions run) of `tokens` over src: ["--gaps-bed", BED, REF] or [REF, GAPS.fa]"""
    a, b = os.path.join(str(cwd), "regions.bed"), os.path.join(str(cwd), "merged.bed")
    for f in (a, b):
        if os.path.exists(f):
            os.remove(f)
    s = _run(tok + list(extra) + src, cwd, **env)
    r = _run(tok + list(extra) + ["--regions-bed", a, "--merged-bed", b] + src, cwd, **env)
    assert r.stdout == b""
    return s.stdout, open(a, "rb").read(), open(b, "rb").read(), s.stderr, r.stderr


def _write_fa(path, seqs):
    with open(path, "w") as f:
        for n, s in seqs:
            f.write(">%s\n" % n.decode() + "".join(s[i:i + 70] + "\n" for i in range(0, len(s), 70)))


BED_MAIN = [b"c2\t2501\t4500", b"c2\t3801\t6000", b"cA\t2001\t3500", b"c2\t100\t150", b"c2\t0\t250", b"c2\t1\t250\tsame_bases\t0\t+", b"", b"c2\t2501\t4500"] + \
           [tc.row(b"c2", 800 + i, 160 + i) for i in range(8)] + [tc.row(b"c10", 9000 - 150, 150), b"c10\t8800\t99999", b"cA\t40\t60"]
BED_SMALL = [b"c2\t100\t150", b"c2\t2501\t3000", b"cA\t1\t99", b"cA\t2001\t2200", b"cA\t2990\t3000", tc.row(b"c10", 9000 - 141, 141)]
BED_MASKED = [b"cA\t4901\t5700", b"cA\t5251\t5400"]


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """The three contigs of test_gpu_regions_cli.py's `planted` set -- name order (c10, c2, cA) is not index order (c2, cA, c10); c2[3000:5000] is planted at
    c10[1000:3000] -- with 1500 N in cA; cA[5000:5600] is soft-masked and holds an IUPAC R, which only BED_MASKED touches.  Everything else is upper-case ACGTN."""
    d = tmp_path_factory.mktemp("tokens_bed_planted")
    rnd = random.Random(20261019)
    seq = {n: "".join(rnd.choice("ACGT") for _ in range(l)) for n, l in (("c2", 12000), ("cA", 8000), ("c10", 9000))}
    seq["c10"] = seq["c10"][:1000] + seq["c2"][3000:5000] + seq["c10"][3000:]
    seq["cA"] = seq["cA"][:2000] + "N" * 1500 + seq["cA"][3500:5000] + seq["cA"][5000:5300].lower() + "R" + seq["cA"][5301:5600].lower() + seq["cA"][5600:]
    seqs = [(n.encode(), seq[n]) for n in ("c2", "cA", "c10")]
    assert [(n, len(s)) for n, s in seqs] == tc.CONTIGS
    _write_fa(d / "ref.fa", seqs)
    for name, lines in (("main", BED_MAIN), ("small", BED_SMALL), ("masked", BED_MASKED)):
        bed = b"\n".join(lines) + b"\n"
        (d / (name + ".bed")).write_bytes(bed); (d / (name + ".fa")).write_bytes(tc.gaps_fasta(bed, seqs))
    tok = ["tokens", "--read-size", "100", "--skip", "20"]
    return dict(d=d, tok=tok, fasta=_all(tok, ["ref.fa", "main.fa"], d), bed=_all(tok, ["--gaps-bed", "main.bed", "ref.fa"], d))


def test_planted_sam_and_regions_are_those_of_the_fasta_run(planted):
    p = planted
    sam, per_gap, merged = p["fasta"][:3]
    assert p["bed"][0] == sam and p["bed"][1] == per_gap and p["bed"][2] == merged
    # what the BED is there for
    rr = tc.rows(b"\n".join(BED_MAIN) + b"\n", tc.CONTIGS)
    toks = tc.tokens([n for _, _, _, n in rr], 100, 20)
    recs = [l.split(b"\t") for l in sam.split(b"\n") if l and not l.startswith(b"@")]
    assert len(toks) > 300 and sorted({f[0] for f in recs}) == sorted({rr[r][0] + b"_%d" % o for r, o in toks})
    assert {(off + s) & 7 for (_, c, s, _), off in ((x, (0, 12000, 20000)[x[1]]) for x in rr[7:15])} == set(range(8))
    assert rr[15][2] + rr[15][3] == 9000 and rr[16][2] + rr[16][3] == 9000 and rr[3][3] < 100 and rr[17][3] < 100      # the last bases of the last contig, twice; no token
    assert rr[4][2:] == rr[5][2:] and rr[0] == rr[6]                                                                        # a = 0 and a = 1; the same row twice
    n_only = [f for f in recs if f[0].startswith(b"cA:2001-3500_")]
    assert len(n_only) == 70 and all(int(f[1]) & 4 and f[9] == b"N" * 100 for f in n_only)                                  # every token of the N row is unmapped
    v, names = rc.sam_intervals(sam, tc.gap_names(b"\n".join(BED_MAIN)))
    assert not [x for x in v if x[0] == 2] and per_gap != merged and per_gap.count(b"\n") > merged.count(b"\n")
    # the same row twice is two groups: its lines stand twice in the per-gap file, once in the merged one
    assert per_gap.count(per_gap[:per_gap.index(b"\n") + 1]) >= 2 and merged.count(per_gap[:per_gap.index(b"\n") + 1]) <= 1


def test_planted_batched_halved_and_with_secondaries(planted):
    p = planted; src = ["--gaps-bed", "main.bed", "ref.fa"]
    want = p["fasta"][:3]
    assert _all(p["tok"], src, p["d"], extra=["-K", "2000"])[:3] == want                   # 20 tokens per batch: rows are split across batches, batches span rows
    h = _all(p["tok"], src, p["d"], AL_TEST_NOMEM_ABOVE=11)
    assert h[:3] == want and b"does not fit the device workspaces" in h[3] and b"does not fit the device workspaces" in h[4]
    sec = ["--secondary=yes"]
    want2 = _all(p["tok"], ["ref.fa", "main.fa"], p["d"], extra=sec)[:3]
    assert want2[0] != want[0] and want2[1] != want[1]
    assert _all(p["tok"], src, p["d"], extra=sec + ["-K", "2000"])[:3] == want2


def test_planted_one_token_per_batch(planted):
    p = planted
    want = _all(p["tok"], ["ref.fa", "small.fa"], p["d"])[:3]
    got = _all(p["tok"], ["--gaps-bed", "small.bed", "ref.fa"], p["d"], extra=["-K", "100"])[:3]
    assert got == want
    n = len(tc.tokens([n for _, _, _, n in tc.rows(b"\n".join(BED_SMALL) + b"\n", tc.CONTIGS)], 100, 20))
    recs = [l.split(b"\t")[0] for l in want[0].split(b"\n") if l and not l.startswith(b"@")]
    assert 20 < n < 40 and len(recs) >= n and len(set(recs)) == n and len({r for r in recs if r.startswith(b"c10:8860-9000_")}) == 3


def test_planted_masked_contig_differs_in_seq_only(planted):
    p = planted
    a = _run(p["tok"] + ["ref.fa", "masked.fa"], p["d"]).stdout.split(b"\n")
    b = _run(p["tok"] + ["--gaps-bed", "masked.bed", "ref.fa"], p["d"]).stdout.split(b"\n")
    assert len(a) == len(b) and a != b
    n_diff = 0
    for x, y in zip(a, b):
        if x.startswith(b"@") or not x:
            assert x == y
            continue
        fx, fy = x.split(b"\t"), y.split(b"\t")
        assert fx[:9] == fy[:9] and fx[10:] == fy[10:]
        assert fy[9] == bytes(c if c in b"ACGT" else ord("N") for c in fx[9].upper())
        n_diff += fx[9] != fy[9]
    assert n_diff > 30 and any(b"R" in x.split(b"\t")[9] for x in a if x and not x.startswith(b"@"))


def test_capi_gives_the_clis_bytes(planted):
    import airlift_amd as A
    p = planted; d = p["d"]
    L = A.load()
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p; libc.fopen.argtypes = [C.c_char_p, C.c_char_p]; libc.fclose.argtypes = [C.c_void_p]
    idx = A.Index(fasta=str(d / "ref.fa"), on_device=0)
    try:
        bed = str(d / "main.bed").encode()
        assert L.al_map_tokens_bed_regions(idx.h, bed, 100, 20, C.byref(idx.mo), 3, None, None, 0) == -1
        fa, fb = libc.fopen(str(d / "capi_r.bed").encode(), b"wb"), libc.fopen(str(d / "capi_m.bed").encode(), b"wb")
        rcode = L.al_map_tokens_bed_regions(idx.h, bed, 100, 20, C.byref(idx.mo), 3, fa, fb, 0)
        libc.fclose(fa); libc.fclose(fb)
        assert rcode == 0
        fs = libc.fopen(str(d / "capi.sam").encode(), b"wb")
        rcode = L.al_map_tokens_bed_file(idx.h, bed, 100, 20, C.byref(idx.mo), 3, fs, None, 0)
        libc.fclose(fs)
        assert rcode == 0
    finally:
        idx.close()
    assert open(d / "capi_r.bed", "rb").read() == p["bed"][1] and open(d / "capi_m.bed", "rb").read() == p["bed"][2]
    assert open(d / "capi.sam", "rb").read() == p["bed"][0]


def test_g10_gaps_bed_is_the_reference_builds_sam(golden_unpacked):
    d = golden_unpacked["g10_gaps_bed"]
    m = json.load(open(os.path.join(d, "meta.json")))
    sam = open(os.path.join(d, "expected.sam"), "rb").read()
    tok = ["tokens", "--read-size", str(m["read_size"]), "--skip", str(m["skip"])]
    got = _all(tok, ["--gaps-bed", m["bed"], m["ref"]], d)
    assert got[0] == sam and sam.count(b"\n") == m["n_sam_lines"]
    bed = open(os.path.join(d, m["bed"]), "rb").read()
    v, names = rc.sam_intervals(sam, tc.gap_names(bed))
    assert len(v) == m["n_tokens"] and got[1] == rc.bed(rc.merge(v, names, True), names) and got[2] == rc.bed(rc.merge(v, names, False), names)
    # the committed GAPS.fa is the BED's by the definition, and the FASTA route over it gives the same three outputs
    seq = "".join(l.strip() for l in open(os.path.join(d, m["ref"])) if not l.startswith(">"))
    assert open(os.path.join(d, m["gaps"]), "rb").read() == tc.gaps_fasta(bed, [(b"MT_human", seq)])
    assert _all(tok, [m["ref"], m["gaps"]], d)[:3] == got[:3]
    # overlapping rows: their own lines per gap, one line merged; the exact copies map where they were cut (a region's last token ends before its last base)
    assert got[1] == b"".join(b"MT_human\t%d\t%d\n" % se for se in ((0, 415), (4000, 4247), (8999, 9694), (9499, 10299), (11999, 12099), (6999, 7344), (16299, 16567)))
    assert got[2] == b"".join(b"MT_human\t%d\t%d\n" % se for se in ((0, 415), (4000, 4247), (6999, 7344), (8999, 10299), (11999, 12099), (16299, 16567)))

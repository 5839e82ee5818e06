"""-m gpu: the --MD / --cs / -Y output options end to end.  The tags are computed on the device (al_kernels_tags.hip) and spliced by
every output path; the output must equal what the fork itself prints with the same options (tests/golden/g8_tags, made by
tests/golden/make_g8_tags.py) byte for byte -- stream driver, host driver, several lanes, one process per rank -- and BAM must decode to
the same records.  Flag-off output is pinned by the existing golden tests."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
META = json.load(open(os.path.join(ROOT, "tests", "golden", "g8_tags", "meta.json")))
CASES = [(s, k) for s in sorted(META["sets"]) for k in sorted(META["sets"][s]["out"])]


def _case(golden_unpacked, name, key):
    g = golden_unpacked["g8_tags"]
    d = g if name == "g8_chimeric" else golden_unpacked[name]
    e = META["sets"][name]
    args = (["-R", e["rg"]] if e.get("rg") else []) + META["flags"][key]
    exp = open(os.path.join(g, "%s__%s.sam" % (name, key)), "rb").read()
    return d, e, args, exp


def _diff(got, exp):
    g, e = got.split(b"\n"), exp.split(b"\n")
    bad = [i for i in range(min(len(g), len(e))) if g[i] != e[i]]
    return "%d vs %d lines, %d differ; first: %s" % (len(g), len(e), len(bad), "\n got %s\n exp %s" % (g[bad[0]][:400], e[bad[0]][:400]) if bad else "")


@pytest.mark.parametrize("name,key", CASES, ids=["%s-%s" % c for c in CASES])
def test_stream_driver_matches_fork(golden_unpacked, name, key):
    d, e, args, exp = _case(golden_unpacked, name, key)
    r = subprocess.run([CLI, "-ax", "sr"] + args + [e["ref"]] + e["reads"], cwd=d, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == exp, _diff(r.stdout, exp)


HOST_CASES = [("g8_chimeric", "MD"), ("g8_chimeric", "Y_cs_long"), ("g8_chimeric", "cs"), ("g3_adversarial", "MD"), ("g1_mt150pe", "Y_cs_long"), ("g4_q_inv", "MD_cs_long")]


@pytest.mark.parametrize("name,key", HOST_CASES, ids=["%s-%s" % c for c in HOST_CASES])
def test_host_driver_matches_fork(golden_unpacked, name, key):
    """AL_HOST_IO=1: reads parsed and SAM formatted on the host (the FASTA / gzip / token path); the tags come from the device all the same."""
    d, e, args, exp = _case(golden_unpacked, name, key)
    r = subprocess.run([CLI, "-ax", "sr", "-K", "20000"] + args + [e["ref"]] + e["reads"], cwd=d, capture_output=True, timeout=300, env=dict(os.environ, AL_HOST_IO="1"))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == exp, _diff(r.stdout, exp)


@pytest.mark.parametrize("name,key", [("g8_chimeric", "Y_cs_long"), ("g3_adversarial", "MD")])
def test_two_lanes_match_fork(golden_unpacked, tmp_path, name, key):
    d, e, args, exp = _case(golden_unpacked, name, key)
    o = str(tmp_path / "multi.sam")
    r = subprocess.run([CLI, "-ax", "sr", "-K", "30000", "--devices", "0,0", "-o", o] + args + [e["ref"]] + e["reads"], cwd=d, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = open(o, "rb").read()
    assert got == exp, _diff(got, exp)


def test_one_process_per_rank_matches_fork(golden_unpacked, tmp_path):
    d, e, args, exp = _case(golden_unpacked, "g1_mt150pe", "Y_cs_long")
    out = tmp_path / "merged.sam"
    env = dict(os.environ, AL_RUN_ID="tags2", AL_RANK_TIMEOUT="120")
    ps = [subprocess.Popen([CLI, "-ax", "sr", "-t", "4", "--device", "0", "--rank", str(r), "--world", "2", "--rendezvous", str(tmp_path), "-o", str(out)] + args + [e["ref"]] + e["reads"],
                           cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env) for r in range(2)]
    outs = [p.communicate(timeout=300) for p in ps]
    assert all(p.returncode == 0 for p in ps), b"\n".join(o[1][-800:] for o in outs).decode()
    assert out.read_bytes() == exp, _diff(out.read_bytes(), exp)


@pytest.mark.parametrize("name,key", [("g8_chimeric", "MD"), ("g8_chimeric", "Y_cs_long"), ("g1_mt150pe", "Y_cs_long")])
def test_bam_decodes_to_the_forks_records(golden_unpacked, name, key):
    from bam_util import read_bam, sam_fields
    d, e, args, exp = _case(golden_unpacked, name, key)
    lines = exp.decode().split("\n")
    body = [l for l in lines if l and not l.startswith("@")]
    for mode in ["--bam", "--sorted-bam"]:
        r = subprocess.run([CLI, "-ax", "sr", mode, "-K", "50000"] + args + [e["ref"]] + e["reads"], cwd=d, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        text, refs, recs, _ = read_bam(r.stdout)
        names = [n for n, _ in refs]
        want = [sam_fields(l, names) for l in body]
        if mode == "--sorted-bam":
            want = [s for s in want if not s["flag"] & 4]
            order = sorted(range(len(want)), key=lambda i: (want[i]["rid"], want[i]["pos"]))
            want = [want[i] for i in order]
        assert len(recs) == len(want)
        for b, s in zip(recs, want):
            for k in ("qname", "flag", "rid", "pos", "mapq", "cigar", "nrid", "npos", "tlen", "qual"):
                assert b[k] == s[k], (mode, k, b, s)
            assert b["seq"] == s["seq"].upper(), (mode, b, s)        # (4-bit BAM bases carry no case)
            assert [t for t in b["tags"] if not isinstance(t, tuple)] == [t for t in s["tags"] if not isinstance(t, tuple)], (mode, b, s)


def test_tokens_with_md_match_the_restatement(golden_unpacked):
    """tokens (reads cut from the gap FASTA on the device) with --MD: the tag of every record equals the Python restatement from POS,
    CIGAR, SEQ and the reference; without the tag the output is the token golden."""
    from tags_util import read_fasta, record_tag
    d = golden_unpacked["g7_tokens"]
    m = json.load(open(os.path.join(d, "meta.json")))
    base = [CLI, "tokens", "--read-size", str(m["read_size"]), "--skip", str(m["skip"])]
    r = subprocess.run(base + ["--MD", m["ref"], m["gaps"]], cwd=d, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    ref = read_fasta(os.path.join(d, m["ref"]))
    n = 0; stripped = []
    for l in r.stdout.decode().split("\n"):
        if not l or l.startswith("@"):
            stripped.append(l); continue
        f = l.split("\t")
        md = [x for x in f[11:] if x.startswith("MD:Z:")]
        want = record_tag(f, ref, "MD")
        if want is not None:
            assert md == ["MD:Z:" + want], (f[0], md, want); n += 1
        stripped.append("\t".join(x for x in f if not x.startswith("MD:Z:")))
    assert n > 300
    assert "\n".join(stripped).encode() == open(os.path.join(d, "expected.sam"), "rb").read()


def test_gen_md_on_a_device_built_index_equals_the_cli_tag(golden_unpacked):
    """al_gen_MD with an index that lives only on the device (the reference window is copied from HBM) gives, for the records al_map_frag
    returns, the MD:Z strings the fork printed for the same reads."""
    import ctypes as C
    import airlift_amd as A
    d, e, args, exp = _case(golden_unpacked, "g8_chimeric", "MD")
    reads = A.read_fastx(os.path.join(d, "chim.fq"))
    golden = {}
    for l in exp.decode().split("\n"):
        if l and not l.startswith("@"):
            f = l.split("\t")
            golden.setdefault(f[0], []).append([x[5:] for x in f[11:] if x.startswith("MD:Z:")])
    idx = A.Index(fasta=os.path.join(d, "chim.fa"), on_device=0)
    ctx = A.Context(idx)
    L = A.load()
    n_checked = 0
    for i in range(0, 300, 9):
        name, seq = reads[0][i], reads[1][i]
        ql = (C.c_int * 1)(len(seq)); sq = (C.c_char_p * 1)(seq)
        nr = (C.c_int * 1)(); rg = (C.POINTER(A.Reg) * 1)()
        L.al_map_frag(idx.h, 1, ql, sq, nr, rg, ctx.h, C.byref(idx.mo), name)
        want = golden[name.decode()]
        assert nr[0] == len(want)
        for k in range(nr[0]):
            got = A.gen_tag(idx.h, rg[0][k], seq, "MD").decode()
            assert [got] == want[k], (name, k, got, want[k]); n_checked += 1
    ctx.close(); idx.close()
    assert n_checked > 40


def test_map_frag_with_eqx_returns_eq_x_cigars(golden_unpacked):
    """al_map_frag in a context whose options carry AL_F_EQX returns the =/X CIGARs the fork prints with --eqx."""
    import ctypes as C
    import airlift_amd as A
    d, e, args, exp = _case(golden_unpacked, "g8_chimeric", "eqx")
    want = {}
    for l in exp.decode().split("\n"):
        if l and not l.startswith("@"):
            f = l.split("\t")
            want.setdefault(f[0], []).append(f[5])
    names, seqs, _ = A.read_fastx(os.path.join(d, "chim.fq"))
    idx = A.Index(fasta=os.path.join(d, "chim.fa"), on_device=0)
    idx.mo.flag |= A.AL_F_EQX
    ctx = A.Context(idx)
    L = A.load()
    n_eqx = 0
    for i in range(0, 300, 7):
        ql = (C.c_int * 1)(len(seqs[i])); sq = (C.c_char_p * 1)(seqs[i])
        nr = (C.c_int * 1)(); rg = (C.POINTER(A.Reg) * 1)()
        L.al_map_frag(idx.h, 1, ql, sq, nr, rg, ctx.h, C.byref(idx.mo), names[i])
        w = want[names[i].decode()]
        assert nr[0] == len(w)
        for k in range(nr[0]):
            r = rg[0][k]
            ops = "".join("%d%s" % (r.cigar[j] >> 4, "MIDNSHP=XB"[r.cigar[j] & 0xf]) for j in range(r.n_cigar))
            assert "M" not in ops and ops in w[k], (names[i], k, ops, w[k]); n_eqx += 1
    ctx.close(); idx.close()
    assert n_eqx > 40


def _synth(tmp_path, config, pairs):
    import gen_synth
    d = str(tmp_path / config)
    gen_synth.generate(config, d, pairs=pairs)
    return d


@pytest.mark.parametrize("config,pairs", [("tiny", 100000), ("c2r", 100000)], ids=["tiny_100k", "repeats_100k"])
def test_synthetic_sample_tags_and_flag_off_equivalence(tmp_path, config, pairs):
    """A 100 k-pair synthetic sample (and a repeat-rich one) in several batches: with --MD --eqx -Y every MD:Z equals the restatement from
    POS, CIGAR, SEQ and the FASTA; with --cs=long every cs:Z does; and undoing the options gives exactly the flag-off output."""
    from tags_util import read_fasta, record_tag, strip_options
    d = _synth(tmp_path, config, pairs)
    base = [CLI, "-ax", "sr", "-t", "8", "-K", "5000000"]
    ins = ["ref.fa", "reads_1.fq", "reads_2.fq"]
    off = subprocess.run(base + ins, cwd=d, capture_output=True, timeout=600)
    assert off.returncode == 0, off.stderr.decode()[-2000:]
    ref = read_fasta(os.path.join(d, "ref.fa"))
    for flags, kind, long_cs in [(["--MD", "--eqx", "-Y"], "MD", False), (["--cs=long"], "cs", True)]:
        on = subprocess.run(base + flags + ins, cwd=d, capture_output=True, timeout=600)
        assert on.returncode == 0, on.stderr.decode()[-2000:]
        lines = on.stdout.decode().split("\n")
        n = 0
        for l in lines:
            if l and not l.startswith("@"):
                f = l.split("\t")
                want = record_tag(f, ref, kind, long_cs)
                if want is not None:
                    got = [x[5:] for x in f[11:] if x.startswith(kind + ":Z:")]
                    assert got == [want], (f[0], f[1], f[5], got, want); n += 1
        assert n > pairs
        assert "\n".join(l if not l or l.startswith("@") else strip_options(l) for l in lines).encode() == off.stdout


def test_remap_with_md_and_eqx(golden_unpacked, tmp_path):
    """remap (its own argv loop) takes the options: every MD:Z equals the restatement, and undoing them gives the flag-off remap output."""
    from test_gpu_remap import _cigar, write_bam
    from tags_util import read_fasta, record_tag, strip_options
    d = golden_unpacked["g1_mt150pe"]
    m = json.load(open(os.path.join(d, "meta.json")))
    refs, recs = [], []
    for line in open(os.path.join(d, "expected.sam")):
        f = line.rstrip("\n").split("\t")
        if line.startswith("@SQ"):
            refs.append((f[1][3:], int(f[2][3:])))
        if line.startswith("@") or int(f[1]) & 0x900 or f[2] == "*":
            continue
        recs.append(([r[0] for r in refs].index(f[2]), int(f[3]) - 1, int(f[4]), int(f[1]), _cigar(f[5]) if f[5] != "*" else [], f[0], len(f[9])))
    recs.sort(key=lambda r: (r[0], r[1]))
    bam = str(tmp_path / "old.bam"); write_bam(bam, refs, recs)
    bed = str(tmp_path / "regions.bed")
    open(bed, "w").write("%s\t200\t%d\n" % (refs[0][0], refs[0][1] - 100))
    ref = os.path.join(d, m["ref"]); fq = [os.path.join(d, r) for r in m["reads"]]
    out = {}
    for key, fl in [("off", []), ("on", ["--MD", "--eqx"])]:
        o = str(tmp_path / (key + ".sam"))
        r = subprocess.run([CLI, "remap", "--noprune"] + fl + ["-o", o, ref, bam, bed, fq[0], fq[1]], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-1500:]
        out[key] = open(o).read()
    seqs = read_fasta(ref)
    lines = out["on"].split("\n"); n = 0
    for l in lines:
        if l and not l.startswith("@"):
            f = l.split("\t"); want = record_tag(f, seqs, "MD")
            if want is not None:
                assert [x[5:] for x in f[11:] if x.startswith("MD:Z:")] == [want]; n += 1
    assert n > 500
    assert "\n".join(l if not l or l.startswith("@") else strip_options(l) for l in lines) == out["off"]

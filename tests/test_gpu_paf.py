"""-m gpu: PAF output (--paf, -c, --cs, --paf-no-hit), --secondary and the map-only mode end to end.  Every output must equal what the
fork itself prints with the same options (tests/golden/g9_paf, made by tests/golden/make_g9_paf.py) byte for byte, all lines, in order
-- through the stream driver, the host driver, two lanes and one process per rank.  `--paf` without -c / --cs runs no base-level
alignment: its goldens differ from the aligned ones in the number of lines (a run that left the extension DP on cannot pass)."""
import ctypes as C
import gzip
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
G9 = os.path.join(ROOT, "tests", "golden", "g9_paf")
META = json.load(open(os.path.join(G9, "meta.json")))
PAF_CASES = [(s, k) for s in sorted(META["sets"]) for k in sorted(META["sets"][s]["out"]) if not k.startswith("sam_")]
SAM_CASES = [(s, k) for s in sorted(META["sets"]) for k in sorted(META["sets"][s]["out"]) if k.startswith("sam_")]
IDS = lambda cs: ["%s-%s" % c for c in cs]


def _case(golden_unpacked, name, key):
    """working directory with the inputs, the set's entry, the options after `-x sr`, the fork's output"""
    e = META["sets"][name]
    d = golden_unpacked["g8_tags"] if name == "g8_chimeric" else golden_unpacked[name]
    exp = gzip.open(os.path.join(G9, e["out"][key]["file"]), "rb").read()
    args = (["-R", e["rg"]] if e.get("rg") else []) + (["-a"] if key.startswith("sam_") else ["--paf"]) + META["flags"][key]
    return d, e, args, exp


def _diff(got, exp):
    g, e = got.split(b"\n"), exp.split(b"\n")
    bad = [i for i in range(min(len(g), len(e))) if g[i] != e[i]]
    return "%d vs %d lines, %d differ; first: %s" % (len(g), len(e), len(bad), "\n got %s\n exp %s" % (g[bad[0]][:400], e[bad[0]][:400]) if bad else "")


def test_goldens_are_the_ones_the_generator_recorded():
    """md5 and line counts of every committed golden as meta.json has them (the counts of the feature request: 3137 map-only lines
    against 2962 aligned ones on g3, 128 no-hit lines, 2240 / 2028 secondaries, ...)."""
    import hashlib
    for name, e in META["sets"].items():
        for key, o in e["out"].items():
            text = gzip.open(os.path.join(G9, o["file"]), "rb").read()
            assert hashlib.md5(text).hexdigest() == o["md5"], (name, key)
            lines = [l for l in text.split(b"\n") if l and not (key.startswith("sam_") and l.startswith(b"@"))]
            assert len(lines) == o["n_lines"] and sum(b"\ttp:A:S" in l for l in lines) == o["n_tpS"], (name, key)
    g3 = META["sets"]["g3_adversarial"]["out"]
    assert (g3["paf"]["n_lines"], g3["c"]["n_lines"], g3["c"]["n_cg"], g3["c"]["n_de"], g3["cs"]["n_cs"], g3["nohit"]["n_lines"], g3["nohit"]["n_no_hit"]) == (3137, 2962, 2962, 2962, 2962, 3265, 128)
    assert (g3["sec"]["n_lines"], g3["sec"]["n_tpS"], g3["c_sec"]["n_lines"], g3["c_sec"]["n_tpS"]) == (5377, 2240, 4990, 2028)
    assert g3["MD"]["md5"] == g3["paf"]["md5"] and g3["MD"]["n_MD"] == 0
    g6 = META["sets"]["g6_repeats"]["out"]
    assert (g6["paf"]["n_lines"], g6["c"]["n_lines"], g6["sec"]["n_lines"], g6["sec"]["n_tpS"], g6["c_sec"]["n_lines"], g6["c_sec"]["n_tpS"]) == (1056, 1000, 2667, 1611, 2443, 1443)
    g2 = META["sets"]["g2_100se"]["out"]
    assert (g2["paf"]["n_lines"], g2["c"]["n_lines"], g2["sec"]["n_lines"], g2["sec"]["n_tpS"]) == (1493, 1493, 2431, 938)


@pytest.mark.parametrize("name,key", PAF_CASES, ids=IDS(PAF_CASES))
def test_stream_driver_matches_fork(golden_unpacked, name, key):
    d, e, args, exp = _case(golden_unpacked, name, key)
    r = subprocess.run([CLI, "-x", "sr"] + args + [e["ref"]] + e["reads"], cwd=d, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"ignored" not in r.stderr
    assert r.stdout == exp, _diff(r.stdout, exp)


@pytest.mark.parametrize("name,key", PAF_CASES, ids=IDS(PAF_CASES))
def test_host_driver_matches_fork(golden_unpacked, name, key):
    """AL_HOST_IO=1: reads parsed and lines formatted on the host (al_write_paf); several batches."""
    d, e, args, exp = _case(golden_unpacked, name, key)
    r = subprocess.run([CLI, "-ax", "sr", "-K", "20000"] + args + [e["ref"]] + e["reads"], cwd=d, capture_output=True, timeout=300, env=dict(os.environ, AL_HOST_IO="1"))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == exp, _diff(r.stdout, exp)


@pytest.mark.parametrize("name,key", PAF_CASES, ids=IDS(PAF_CASES))
def test_two_lanes_match_fork(golden_unpacked, tmp_path, name, key):
    d, e, args, exp = _case(golden_unpacked, name, key)
    o = str(tmp_path / "multi.paf")
    r = subprocess.run([CLI, "-x", "sr", "-K", "30000", "--devices", "0,0", "-o", o] + args + [e["ref"]] + e["reads"], cwd=d, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = open(o, "rb").read()
    assert got == exp, _diff(got, exp)


@pytest.mark.parametrize("name,key", PAF_CASES, ids=IDS(PAF_CASES))
def test_one_process_per_rank_matches_fork(golden_unpacked, tmp_path, name, key):
    """Two ranks on one GPU into one file: no header, so rank 0 writes nothing ahead of its first batch."""
    d, e, args, exp = _case(golden_unpacked, name, key)
    out = tmp_path / "merged.paf"
    env = dict(os.environ, AL_RUN_ID="paf_%s_%s" % (name, key), AL_RANK_TIMEOUT="120")
    ps = [subprocess.Popen([CLI, "-x", "sr", "-t", "4", "--device", "0", "--rank", str(r), "--world", "2", "--rendezvous", str(tmp_path), "-o", str(out)] + args + [e["ref"]] + e["reads"],
                           cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env) for r in range(2)]
    outs = [p.communicate(timeout=300) for p in ps]
    assert all(p.returncode == 0 for p in ps), b"\n".join(o[1][-800:] for o in outs).decode()
    assert out.read_bytes() == exp, _diff(out.read_bytes(), exp)


def test_md_alone_does_not_turn_the_alignment_on(golden_unpacked):
    """--paf --MD: the fork's MM_F_OUT_MD without MM_F_CIGAR -- the map-only lines, byte for byte, and no MD:Z."""
    d, e, args, exp = _case(golden_unpacked, "g3_adversarial", "MD")
    assert exp == _case(golden_unpacked, "g3_adversarial", "paf")[3] and b"MD:Z" not in exp
    r = subprocess.run([CLI, "-x", "sr"] + args + ["--eqx", "-Y", e["ref"]] + e["reads"], cwd=d, capture_output=True, timeout=300)   # (--eqx and -Y have nothing to act on either)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == exp, _diff(r.stdout, exp)


@pytest.mark.parametrize("name,key", SAM_CASES, ids=IDS(SAM_CASES))
def test_secondary_yes_with_sam_and_bam(golden_unpacked, name, key):
    """--secondary=yes clears the sr preset's AL_F_NO_PRINT_2ND for the SAM writers (stream and host driver) and the BAM writer; -c
    changes nothing with SAM output (as in the fork)."""
    from bam_util import read_bam, sam_fields
    d, e, args, exp = _case(golden_unpacked, name, key)
    for extra, env in [([], None), (["-c"], None), (["-K", "20000"], dict(os.environ, AL_HOST_IO="1"))]:
        r = subprocess.run([CLI, "-x", "sr"] + args + extra + [e["ref"]] + e["reads"], cwd=d, capture_output=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert r.stdout == exp, _diff(r.stdout, exp)
    r = subprocess.run([CLI, "-x", "sr"] + args + ["--secondary=no", e["ref"]] + e["reads"], cwd=d, capture_output=True, timeout=300)       # the last one wins: the plain golden
    assert r.returncode == 0 and r.stdout == open(os.path.join(d, "expected.sam"), "rb").read()
    body = [l for l in exp.decode().split("\n") if l and not l.startswith("@")]
    r = subprocess.run([CLI, "-x", "sr", "--bam", "-K", "50000"] + args + [e["ref"]] + e["reads"], cwd=d, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    text, refs, recs, _ = read_bam(r.stdout)
    names = [n for n, _ in refs]
    want = [sam_fields(l, names) for l in body]
    assert len(recs) == len(want) and sum(1 for b in recs if b["flag"] & 0x100) == META["sets"][name]["out"][key]["n_tpS"] > 0
    for b, s in zip(recs, want):
        for k in ("qname", "flag", "rid", "pos", "mapq", "cigar", "nrid", "npos", "tlen", "qual"):
            assert b[k] == s[k], (k, b, s)
        assert b["seq"] == s["seq"].upper(), (b, s)
        assert [t for t in b["tags"] if not isinstance(t, tuple)] == [t for t in s["tags"] if not isinstance(t, tuple)], (b, s)


def _map_frags(A, idx, ctx, n_segs, seqs, names):
    """al_map_frag fragment by fragment: [(read name, read length, rep_len is not returned by this entry point, [Reg...])] in read order"""
    L = A.load()
    out, i = [], 0
    for ns in n_segs:
        ql = (C.c_int * ns)(*[len(s) for s in seqs[i:i + ns]]); sq = (C.c_char_p * ns)(*seqs[i:i + ns])
        nr = (C.c_int * ns)(); rg = (C.POINTER(A.Reg) * ns)()
        L.al_map_frag(idx.h, ns, ql, sq, nr, rg, ctx.h, C.byref(idx.mo), names[i])
        for j in range(ns):
            out.append((names[i + j], len(seqs[i + j]), [rg[j][k] for k in range(nr[j])]))
        i += ns
    return out


@pytest.mark.parametrize("name", ["g3_adversarial", "g2_100se"])
def test_map_frag_map_only_returns_the_chain_level_hits(golden_unpacked, name):
    """al_map_frag under AL_F_OUT_PAF without AL_F_CIGAR: hits with n_cigar == 0, cigar == NULL, dp_* zero, mlen / blen from
    mm_reg_set_coor; their al_write_paf text is the fork's map-only output with secondaries (every hit is returned, all lines compared)."""
    import airlift_amd as A
    from gpu_util import load_fragments
    d, e, args, exp = _case(golden_unpacked, name, "sec")
    m, n_segs, seqs, names, _ = load_fragments(d)
    idx = A.Index(fasta=os.path.join(d, e["ref"]), on_device=0)
    idx.mo.flag = (idx.mo.flag & ~(A.AL_F_CIGAR | 0x008)) | A.AL_F_OUT_PAF
    A.load().al_mapopt_update(C.byref(idx.mo), idx.h)
    ctx = A.Context(idx)
    got = []
    rl = {}
    for l in exp.split(b"\n"):      # rl:i: is per fragment and al_map_frag does not return it: taken from the golden line of the same read
        if l:
            rl[l.split(b"\t")[0]] = int(re.search(rb"\trl:i:(\d+)", l).group(1))
    for nm, ln, regs in _map_frags(A, idx, ctx, n_segs, seqs, names):
        for r in regs:
            assert r.n_cigar == 0 and not r.cigar and (r.dp_score, r.dp_max, r.dp_max2, r.n_ambi) == (0, 0, 0, 0) and 0 < r.mlen <= r.blen
            got.append(A.write_paf(idx.h, nm, ln, r, 0, rl.get(nm, 0)))
    ctx.close(); idx.close()
    assert b"".join(got) == exp, _diff(b"".join(got), exp)


def test_batch_api_map_only_equals_map_frag(golden_unpacked):
    """al_batch_upload / al_batch_run / al_batch_fetch under the same flags: the same hits, and rep_len as the fork prints it."""
    import airlift_amd as A
    from gpu_util import load_fragments
    d, e, args, exp = _case(golden_unpacked, "g6_repeats", "sec")
    m, n_segs, seqs, names, _ = load_fragments(d)
    idx = A.Index(fasta=os.path.join(d, e["ref"]), on_device=0)
    idx.mo.flag = (idx.mo.flag & ~(A.AL_F_CIGAR | 0x008)) | A.AL_F_OUT_PAF
    A.load().al_mapopt_update(C.byref(idx.mo), idx.h)
    ctx = A.Context(idx)
    ctx.upload(n_segs, seqs, names); ctx.run()
    n_regs, regs, rep = ctx.fetch()
    got, i = [], 0
    for f, ns in enumerate(n_segs):
        for j in range(ns):
            for k in range(n_regs[i + j]):
                r = regs[i + j][k]
                assert r.n_cigar == 0 and not r.cigar
                got.append(A.write_paf(idx.h, names[i + j], len(seqs[i + j]), r, 0, int(rep[f])))
        i += ns
    st = ctx.stat()
    ctx.close(); idx.close()
    assert b"".join(got) == exp, _diff(b"".join(got), exp)
    stages = {A.load().al_stage_name(k).decode(): st.ms_kernel[k] for k in range(st.n_stage)}
    assert "map_only" in stages and all(stages[k] == 0 or stages[k] < 0.02 for k in stages if k.startswith("ext_")) and st.n_cigar == 0       # the extension stage did not run


def test_paf_c_agrees_with_the_sam_golden_on_g1(golden_unpacked):
    """Cross-check of the two writers on g1: every --paf -c line agrees with the primary record of the existing SAM golden (same read,
    same order) in strand, target, rs (= POS - 1), MAPQ, NM, AS and cg:Z (= CIGAR without its clips)."""
    from gpu_util import qname_len
    d, e, args, exp = _case(golden_unpacked, "g1_mt150pe", "c")
    r = subprocess.run([CLI, "-x", "sr"] + args + [e["ref"]] + e["reads"], cwd=d, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    paf = [l.split("\t") for l in r.stdout.decode().split("\n") if l]
    sam = [l.split("\t") for l in open(os.path.join(d, "expected.sam")).read().split("\n") if l and not l.startswith("@")]
    sam = [f for f in sam if not int(f[1]) & 0x904]                          # primary records of mapped reads
    assert len(paf) == len(sam) == META["sets"]["g1_mt150pe"]["out"]["c"]["n_lines"]
    tag = lambda f, t: [x[5:] for x in f if x.startswith(t)]
    for p, s in zip(paf, sam):
        assert p[0].encode()[:qname_len(p[0].encode())] == s[0].encode()        # (PAF keeps a /1 /2 suffix, SAM drops it; g1's names have none)
        assert p[4] == "+-"[(int(s[1]) >> 4) & 1] and p[5] == s[2] and int(p[7]) == int(s[3]) - 1 and p[11] == s[4]
        assert tag(p[12:], "NM:i:") == tag(s[11:], "NM:i:") and tag(p[12:], "AS:i:") == tag(s[11:], "AS:i:")
        assert tag(p[12:], "cg:Z:") == [re.sub(r"\d+[SH]", "", s[5])]


def _paf_from_sam(sam_text, fq_names, fq_lens, ctg_len):
    """The PAF text of a `--paf -c --cs` run restated from the SAM text (--cs) of the same reads: a line per mapped record, in order.
    qs / qe from the clips and the strand, re from the CIGAR, blen = M + I + D columns - nn, mlen = blen - (NM - nn) (align.c mm_update_extra:
    a column with an ambiguous base counts in nn only, and NM = blen - mlen + nn), the tags in write_tags' order, rl, cg = CIGAR without clips, cs."""
    from gpu_util import qname_len
    out = []
    it = iter((n, l, i & 1) for i, (n, l) in enumerate(zip(fq_names, fq_lens)))      # reads in input order: name, length, mate
    cur = None
    for l in sam_text.split("\n"):
        if not l or l.startswith("@"):
            continue
        f = l.split("\t")
        flag = int(f[1])
        while cur is None or cur[0][:qname_len(cur[0].encode())] != f[0] or cur[2] != (0 if flag & 0x40 else 1):     # (SAM drops a /1 /2 suffix, PAF keeps it)
            cur = next(it)
        if flag & 4:
            continue
        ops = [(int(n), o) for n, o in re.findall(r"(\d+)([MIDNSHP=X])", f[5])]
        lead = ops[0][0] if ops[0][1] in "SH" else 0
        trail = ops[-1][0] if ops[-1][1] in "SH" else 0
        core = [(n, o) for n, o in ops if o not in "SH"]
        L = cur[1]
        rev = (flag >> 4) & 1
        qs, qe = (trail, L - lead) if rev else (lead, L - trail)
        rs = int(f[3]) - 1
        re_ = rs + sum(n for n, o in core if o in "MDN=X")
        tags = dict((x[:5], x[5:]) for x in f[11:])
        blen = sum(n for n, o in core if o in "MID=X") - int(tags["nn:i:"])
        mlen = blen - (int(tags["NM:i:"]) - int(tags["nn:i:"]))
        keep = [x for x in f[11:] if x[:5] in ("NM:i:", "ms:i:", "AS:i:", "nn:i:", "tp:A:", "cm:i:", "s1:i:", "s2:i:", "de:f:", "zd:i:")]
        out.append("\t".join([cur[0], str(L), str(qs), str(qe), "+-"[rev], f[2], str(ctg_len[f[2]]), str(rs), str(re_), str(mlen), str(blen), f[4]] + keep +
                             ["rl:i:" + tags["rl:i:"], "cg:Z:" + "".join("%d%s" % c for c in core), "cs:Z:" + tags["cs:Z:"]]))
    return "\n".join(out) + "\n"


def test_synthetic_sample_paf_restatement_and_batch_independence(tmp_path):
    """A 100 k-pair synthetic sample.  (1) `--paf -c --cs` equals the restatement of its lines from the SAM text (`-a --cs`) of the same
    run.  (2) Map-only output does not depend on the batching: the default batches against batches of 7 pairs and of 1 pair.  The two
    small batch sizes run on the first 3000 pairs of the same files (a batch costs milliseconds of launches and synchronisations whatever
    it holds: 100 000 one-pair batches would take minutes of GPU time and prove nothing more) and are compared with the default run's
    lines for those reads; a run of 7-pair batches over the whole sample is compared as well."""
    import gen_synth
    from tags_util import read_fasta
    import airlift_amd as A
    d = str(tmp_path / "tiny")
    gen_synth.generate("tiny", d, pairs=100000)
    ins = ["ref.fa", "reads_1.fq", "reads_2.fq"]
    base = [CLI, "-x", "sr", "-t", "8", "-K", "5000000"]
    run = lambda args, env=None, files=ins: subprocess.run(base + args + files, cwd=d, capture_output=True, timeout=900, env=env)
    sam = run(["-a", "--cs"]); assert sam.returncode == 0, sam.stderr.decode()[-2000:]
    paf = run(["--paf", "-c", "--cs"]); assert paf.returncode == 0, paf.stderr.decode()[-2000:]
    n1, s1, _ = A.read_fastx(os.path.join(d, "reads_1.fq")); n2, s2, _ = A.read_fastx(os.path.join(d, "reads_2.fq"))
    names = [x.decode() for p in zip(n1, n2) for x in p]; lens = [len(x) for p in zip(s1, s2) for x in p]
    ctg_len = {k: len(v) for k, v in read_fasta(os.path.join(d, "ref.fa")).items()}
    want = _paf_from_sam(sam.stdout.decode(), names, lens, ctg_len)
    assert want.count("\n") > 190000
    assert paf.stdout.decode() == want, _diff(paf.stdout, want.encode())
    # map-only
    mo = run(["--paf"]); assert mo.returncode == 0, mo.stderr.decode()[-2000:]
    assert mo.stdout.count(b"\n") > 190000 and b"cg:Z" not in mo.stdout and b"NM:i" not in mo.stdout and mo.stdout != paf.stdout
    b7 = run(["--paf"], dict(os.environ, AL_BATCH_READS="14")); assert b7.returncode == 0, b7.stderr.decode()[-2000:]
    assert b7.stdout == mo.stdout, _diff(b7.stdout, mo.stdout)
    head = 3000
    for k in (1, 2):
        with open(os.path.join(d, "reads_%d.fq" % k), "rb") as f, open(os.path.join(d, "head_%d.fq" % k), "wb") as o:
            o.write(b"".join(f.readline() for _ in range(4 * head)))
    first = set(x.encode() for x in names[:2 * head])
    want_head = b"".join(l + b"\n" for l in mo.stdout.split(b"\n") if l and l.split(b"\t", 1)[0] in first)
    for reads_per_batch in ("2", "14"):
        r = run(["--paf"], dict(os.environ, AL_BATCH_READS=reads_per_batch), ["ref.fa", "head_1.fq", "head_2.fq"])
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert r.stdout == want_head, _diff(r.stdout, want_head)


def test_remap_writes_paf(golden_unpacked, tmp_path):
    """remap (its own argv loop) takes --paf -c --secondary=yes: the pairs' and the singletons' output equal the aligner run with the same
    options on the files the step-by-step extraction writes; no header."""
    from test_extract_cpu import write_bam
    from test_gpu_remap import _cigar
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
    open(bed, "w").write("".join("%s\t%d\t%d\n" % (refs[0][0], b, e) for b, e in ((200, 3000), (2500, 6000), (9000, refs[0][1] - 100))))
    fq = [os.path.join(d, r) for r in m["reads"]]
    rows = subprocess.run([CLI, "extract-reads", "--noprune", bam, bed], capture_output=True, check=True).stdout
    open(tmp_path / "rows.bed", "wb").write(rows)
    subprocess.run([CLI, "extract-sequence", fq[0], fq[1], str(tmp_path / "rows.bed"), str(tmp_path)], capture_output=True, check=True)
    ref = os.path.join(d, m["ref"])
    opts = ["--paf", "-c", "--secondary=yes"]
    exp_p = subprocess.run([CLI, "-x", "sr"] + opts + [ref, str(tmp_path / "reads_1.fastq"), str(tmp_path / "reads_2.fastq")], capture_output=True, check=True).stdout
    exp_s = subprocess.run([CLI, "-x", "sr"] + opts + [ref, str(tmp_path / "singletons.fastq")], capture_output=True, check=True).stdout
    r = subprocess.run([CLI, "remap", "--noprune"] + opts + ["-R", "@RG\\tID:x\\tSM:y", "-o", str(tmp_path / "p.paf"), "--singletons", str(tmp_path / "s.paf"), ref, bam, bed, fq[0], fq[1]], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    got_p = open(tmp_path / "p.paf", "rb").read()
    assert got_p == exp_p and exp_p.count(b"\n") > 500 and not got_p.startswith(b"@") and b"\tcg:Z:" in got_p
    assert open(tmp_path / "s.paf", "rb").read() == exp_s

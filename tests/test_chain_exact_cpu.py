"""chain-exact without a GPU.  The plain restatement of chainexact_cases.py must give the bytes the reference's script wrote for every g12 golden case;
al_dbg_chainexact_host (the kernels' host twin) must equal the restatement on every generated case; `chain-exact --host` must write the golden bytes in both
modes, and feed chain-beds; every input of the refusal list is refused by message with exit status 1, and what the script merely skips in verify is skipped."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import pytest

import chainexact_cases as cx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
GOLDEN = cx.golden()
IDS = [g[0] for g in GOLDEN]


def _run(args, cwd):
    return subprocess.run([CLI, "chain-exact"] + args, cwd=str(cwd), capture_output=True, timeout=120)


def _lib():
    import airlift_amd as A
    return A.load()


def test_golden_files_are_the_recorded_ones():
    meta = json.load(open(os.path.join(cx.G12, "meta.json")))
    assert sorted(meta) == sorted(IDS) and {"worked", "minus", "order", "ends", "fold", "letters", "random"} <= set(IDS)
    for name, files in meta.items():
        for fn, md5 in files.items():
            assert hashlib.md5(open(cx.golden_path(fn), "rb").read()).hexdigest() == md5, fn   # (random's inputs: made again, the bytes the script read)
    old, _, chain = cx.random_pair()
    assert len(old) == 5 and all(100000 <= len(s) <= 300000 for _, s in old) and 250 <= sum(1 for l in chain.split("\n") if l[:1].isdigit()) <= 400


@pytest.mark.parametrize("case", GOLDEN, ids=IDS)
def test_restatement_gives_the_scripts_bytes(case):
    name, p, want = case
    old, new, chain = (open(p[k]).read() for k in ("old", "new", "chain"))
    for mode in ("verify", "build"):
        assert cx.restate(mode, old, new, chain) == want[mode], mode
    if name == "worked":
        assert want["build"] == b"chain\t5\tx\t2002\t+\t1\t1999\tx\t2008\t+\t1\t2004\t1\n149\t3\t3\n646\t2\t7\n394\t91\t91\n713\n"
        assert want["verify"].count(b"mismatch: 5 errors in 800 block") == 1 and want["verify"].count(b"mismatch: 4 errors in 1200 block") == 1
    if name == "minus":
        assert want["verify"] == b"PASS VERIFICATION\n" and b"-" in want["build"].split(b"\n")[0]
    if name == "order":
        assert [l.split(b"\t")[12] for l in want["build"].split(b"\n") if l.startswith(b"chain")] == [b"1", b"4", b"3", b"2"]


def _cases():
    out = list(cx.synthetic(_lib().al_dbg_chainexact_tile()))
    for name, p, _ in GOLDEN:
        for mode in ("verify", "build"):
            case, _ = cx.table(open(p["old"]).read(), open(p["new"]).read(), open(p["chain"]).read(), mode)
            out.append(("g12_%s_%s" % (name, mode), case, 100 if mode == "build" else 0))
    return out


def test_twin_equals_the_restatement_on_every_case():
    L = _lib()
    assert L.al_dbg_chainexact_tile() >= 64
    for name, case, M in _cases():
        build = M > 0
        assert cx.tap(L.al_dbg_chainexact_host, case, M or 100, build) == cx.model(case, M or 100, build), name
    c = cx.minus_with_an_R(L.al_dbg_chainexact_tile())
    assert cx.model(c)[4] == 1 and cx.tap(L.al_dbg_chainexact_host, c) == ([0, 0], [], [], [], 1)
    # a table that breaks what the table builder guarantees is refused, not read
    bad = cx.Case(b"ACGT", b"ACGT", [(0, 5, 0, 0, 0)], [(0, 0, 0)])
    with pytest.raises(AssertionError):
        cx.tap(L.al_dbg_chainexact_host, bad)


@pytest.mark.parametrize("case", GOLDEN, ids=IDS)
def test_chain_exact_host_writes_the_scripts_bytes(case, tmp_path):
    name, p, want = case
    for mode in ("verify", "build"):
        r = _run([mode, "--host", p["old"], p["new"], p["chain"]], tmp_path)
        assert r.returncode == 0 and r.stdout == want[mode], (mode, r.stderr.decode()[-1000:])
    r = _run(["build", "--host", "-o", "out.chain", "--min-region", "100", p["old"], p["new"], p["chain"]], tmp_path)
    assert r.returncode == 0 and r.stdout == b"" and (tmp_path / "out.chain").read_bytes() == want["build"]
    old, new, chain = (open(p[k]).read() for k in ("old", "new", "chain"))
    for M in (1, 37):
        r = _run(["build", "--host", "--min-region", str(M), p["old"], p["new"], p["chain"]], tmp_path)
        assert r.returncode == 0 and r.stdout == cx.restate("build", old, new, chain, M), M


def test_the_built_chain_file_is_exact_and_feeds_chain_beds(tmp_path):
    p = dict((g[0], g[1]) for g in GOLDEN)["random"]
    assert _run(["build", "--host", "-o", "exact.chain", p["old"], p["new"], p["chain"]], tmp_path).returncode == 0
    r = _run(["verify", "--host", p["old"], p["new"], str(tmp_path / "exact.chain")], tmp_path)
    assert r.returncode == 0 and r.stdout == b"PASS VERIFICATION\n", r.stdout[-500:]
    r = subprocess.run([CLI, "chain-beds", "--host", "--read-size", "100", "--max-errors", "5", "--gaps-out", "-", "--constant-bed", "c.bed", "exact.chain"], cwd=str(tmp_path), capture_output=True)
    assert r.returncode == 0 and r.stdout.count(b"\n") > 50 and (tmp_path / "c.bed").read_bytes().count(b"\n") > 50, r.stderr.decode()[-1000:]


def test_capi_host_flag_opens_no_device(tmp_path):
    L = _lib()
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p; libc.fopen.argtypes = [C.c_char_p, C.c_char_p]; libc.fclose.argtypes = [C.c_void_p]
    name, p, want = GOLDEN[IDS.index("worked")]
    for mode, key in ((0, "verify"), (1, "build")):
        fp = libc.fopen(str(tmp_path / key).encode(), b"wb")
        rc = L.al_chain_exact(p["old"].encode(), p["new"].encode(), p["chain"].encode(), mode, 100, fp, 1, -1)
        libc.fclose(fp)
        assert rc == 0 and (tmp_path / key).read_bytes() == want[key]
    fp = libc.fopen(str(tmp_path / "x").encode(), b"wb")
    assert L.al_chain_exact(p["old"].encode(), p["new"].encode(), p["chain"].encode(), 2, 100, fp, 1, -1) == -1
    assert L.al_chain_exact(p["old"].encode(), p["new"].encode(), p["chain"].encode(), 1, 0, fp, 1, -1) == -1
    assert L.al_chain_exact(p["old"].encode(), p["new"].encode(), p["chain"].encode(), 1, 100, None, 1, -1) == -1
    libc.fclose(fp)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------
SEQ = "ACGTTGCAAGGCTTAC" * 40                                            # 640 bases
HDR = "chain 1 cA 640 + 100 600 qA 640 + 100 600 1\n"
FA_OLD, FA_NEW = ">cA one\n%s\n>cB\n%s\n" % (SEQ, SEQ[:100]), ">qA\n%s\n>qB\n%s\n" % (SEQ, SEQ[:100])
# (chain text, the line that is refused, a word of the reason)
CHAIN_REFUSED = [("100 5 5\n" + HDR + "100\n", 1, "before the first chain header"),
                 (HDR + "100 5\n", 2, "1 or 3 fields"), (HDR + "100 x 5\n", 2, "not a number"), (HDR + "0\n", 2, "size is 0"),
                 (HDR + "100\n200\n", 3, "after the chain's last"),
                 (HDR.replace("cA 640", "cA 2147483648") + "100\n", 1, "tSize is 2^31"),
                 (HDR.replace("640 + 100 600 qA", "640 - 100 600 qA") + "100\n", 1, "tStrand"),
                 (HDR.replace("qA 640 +", "qA 640 x") + "100\n", 1, "qStrand"),
                 (HDR + "600\n", 2, "beyond tSize"), (HDR + "100 500 0\n50\n", 2, "beyond tSize"),
                 ("chain 1 cA 640 + 100\n100\n", 1, "fewer than 12 fields"),
                 (HDR.replace("+ 100 600 1", "+ 100 6oo 1") + "100\n", 1, "qEnd is not a number"),
                 (HDR + "100 5 5\n", 2, "last line is not 1-field"), (HDR + "100 5 5\n\n" + HDR.replace("+ 100 600 qA", "+ 300 600 qA") + "100\n", 2, "last line is not 1-field"),
                 (HDR + "100\n" + HDR.replace(" 1\n", " 2\n") + "50\n", 3, "the same tName, qName and tStart")]


@pytest.mark.parametrize("k", range(len(CHAIN_REFUSED)))
def test_malformed_chain_files_are_refused_by_line(k, tmp_path):
    text, line, word = CHAIN_REFUSED[k]
    (tmp_path / "old.fa").write_text(FA_OLD); (tmp_path / "new.fa").write_text(FA_NEW); (tmp_path / "x.chain").write_text(text)
    for mode in ("verify", "build"):
        for host in (["--host"], []):                                      # refused before a device is opened
            r = _run([mode] + host + ["old.fa", "new.fa", "x.chain"], tmp_path)
            assert r.returncode == 1 and r.stdout == b"", (mode, r.stderr)
            assert ("x.chain:%d: " % line).encode() in r.stderr and word.encode() in r.stderr, r.stderr


def _files(tmp_path, chain, old=FA_OLD, new=FA_NEW):
    (tmp_path / "old.fa").write_text(old); (tmp_path / "new.fa").write_text(new); (tmp_path / "x.chain").write_text(chain)
    return ["old.fa", "new.fa", "x.chain"]


def test_a_minus_strand_and_a_header_without_an_id_are_accepted(tmp_path):
    new = ">qA\n%s\n" % cx.revcomp(SEQ)
    f = _files(tmp_path, "chain 1 cA 640 + 100 600 qA 640 - 100 600\n500\n", new=new)
    r = _run(["build", "--host"] + f, tmp_path)
    assert r.returncode == 0 and r.stdout == b"chain\t1\tcA\t640\t+\t100\t600\tqA\t640\t-\t100\t600\n500\n", r.stderr
    assert _run(["verify", "--host"] + f, tmp_path).stdout == b"PASS VERIFICATION\n"


def test_fasta_files_that_are_refused(tmp_path):
    f = _files(tmp_path, HDR + "500\n", old=FA_OLD + ">cA\nACGT\n")
    r = _run(["verify", "--host"] + f, tmp_path)
    assert r.returncode == 1 and r.stdout == b"" and b"old.fa: the contig 'cA' appears twice" in r.stderr
    for u in "Uu":
        f = _files(tmp_path, HDR + "500\n", new=">qA\n%s\n%s%s\n" % (SEQ[:320], SEQ[320:639], u))
        r = _run(["build", "--host"] + f, tmp_path)
        assert r.returncode == 1 and r.stdout == b"" and b"new.fa:3: a 'U' or 'u'" in r.stderr, r.stderr
    f = _files(tmp_path, HDR + "500\n", old=">Uu\n%s\n" % SEQ)                # (a header line may hold one)
    assert _run(["verify", "--host"] + f, tmp_path).returncode == 0
    f = _files(tmp_path, HDR + "500\n")
    r = _run(["verify", "--host", "none.fa", "new.fa", "x.chain"], tmp_path)
    assert r.returncode == 1 and b"none.fa: cannot be opened" in r.stderr


def test_what_verify_skips_build_refuses(tmp_path):
    """the script's verify skips a chain whose name the FASTA lacks and stops at a block that ends beyond the contig; its build prints a one-line message and
    no chain there: build is refused"""
    for chain, line, word in ((HDR.replace("cA", "cX") + "500\n", 1, "the old FASTA has no contig 'cX'"), (HDR.replace("qA", "qX") + "500\n", 1, "the new FASTA has no contig 'qX'"),
                              ("chain 1 cB 640 + 0 150 qA 640 + 0 150 1\n50 10 10\n90\n", 3, "beyond the old contig"),
                              ("chain 1 cA 640 + 0 150 qB 640 + 0 150 1\n50 10 10\n90\n", 3, "beyond the new contig")):
        f = _files(tmp_path, chain)
        r = _run(["verify", "--host"] + f, tmp_path)
        assert r.returncode == 0 and r.stdout == b"PASS VERIFICATION\n", r.stderr
        r = _run(["build", "--host"] + f, tmp_path)
        assert r.returncode == 1 and r.stdout == b"" and ("x.chain:%d: " % line).encode() in r.stderr and word.encode() in r.stderr, r.stderr


def test_minus_chains_that_are_refused(tmp_path):
    rc = cx.revcomp(SEQ)
    for mode in ("verify", "build"):
        # qSize is larger than the contig: the new-side index starts beyond it; and a block that runs below 0
        for chain, line in (("chain 1 cA 640 + 0 500 qA 700 - 0 500 1\n500\n", 2), ("chain 1 cA 640 + 0 500 qA 640 - 200 500 1\n100 0 0\n400\n", 3)):
            r = _run([mode, "--host"] + _files(tmp_path, chain, new=">qA\n%s\n" % rc), tmp_path)
            assert r.returncode == 1 and r.stdout == b"" and ("x.chain:%d: the block of a '-' chain leaves the new contig" % line).encode() in r.stderr, r.stderr
        # an R among the new side's bases of the second block
        new = rc[:200] + "R" + rc[201:]
        r = _run([mode, "--host"] + _files(tmp_path, "chain 1 cA 640 + 0 600 qA 640 - 0 600 1\n300 0 0\n300\n", new=">qA\n%s\n" % new), tmp_path)
        assert r.returncode == 1 and r.stdout == b"" and b"x.chain:3: a block of a '-' chain compares a new-side byte other than acgtnACGTN" in r.stderr, r.stderr
    # on '+' the same letters compare by identity
    r = _run(["verify", "--host"] + _files(tmp_path, HDR + "500\n", old=">cA\n%s\n" % (SEQ[:200] + "R" + SEQ[201:]), new=">qA\n%s\n" % (SEQ[:200] + "r" + SEQ[201:])), tmp_path)
    assert r.returncode == 0 and r.stdout == b"PASS VERIFICATION\n"


def test_chain_exact_without_its_arguments_prints_its_usage(tmp_path):
    for args in ([], ["verify", "a.fa", "b.fa"], ["make", "a.fa", "b.fa", "c.chain"], ["build", "--host"]):
        r = _run(args, tmp_path)
        assert r.returncode == 1 and b"Usage: airlift-align chain-exact verify|build" in r.stderr
    r = _run(["build", "--min-region", "0", "a.fa", "b.fa", "c.chain"], tmp_path)
    assert r.returncode == 1 and b"--min-region must be positive" in r.stderr

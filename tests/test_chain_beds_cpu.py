"""chain-beds and tokens --chain without a GPU.  `chain-beds --host` (the kernels' host twin) over every g11 golden case must give the bytes the
reference's three scripts wrote; al_dbg_chainreg_host must equal the plain restatement of chainreg_cases.py on every case; every malformed chain file or
merged BED is refused as FILE:LINE: reason in one line, with no device opened and nothing written; the command line of `tokens --chain` refuses what it
cannot serve before the reference is read."""
import ctypes as C
import os
import subprocess

import pytest

import chainreg_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
GOLDEN = cc.golden()
TOK = ["tokens", "--read-size", "100", "--skip", "50"]
CH = ["--chain", "x.chain", "--max-errors", "5"]
NO_GPU = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")


def _run(args, cwd, env=None):
    e = dict(os.environ, **NO_GPU); e.update(env or {})
    return subprocess.run([CLI] + args, capture_output=True, env=e, timeout=60, cwd=str(cwd))


@pytest.mark.parametrize("case", GOLDEN, ids=[c[0] for c in GOLDEN])
def test_chain_beds_host_writes_the_scripts_bytes(case, tmp_path):
    name, _, _, R, E, want = case
    chain = os.path.join(cc.G11, name + ".chain"); merged = os.path.join(cc.G11, name + ".merged.bed")
    r = _run(["chain-beds", "--host", "--read-size", str(R), "--max-errors", str(E), "--gaps-out", "g.bed", "--constant-bed", "c.bed", "--merged-in", merged, "--retired-bed", "r.bed", chain], tmp_path)
    assert r.returncode == 0 and r.stdout == b"" and r.stderr == b"", r.stderr
    for kind, fn in (("gaps", "g.bed"), ("constant", "c.bed"), ("retired", "r.bed")):
        assert (tmp_path / fn).read_bytes() == want[kind], kind
    # one output alone, on stdout; the gaps rows do not need the merged BED
    r = _run(["chain-beds", "--host", "--read-size", str(R), "--max-errors", str(E), "--gaps-out", "-", chain], tmp_path)
    assert r.returncode == 0 and r.stdout == want["gaps"]
    r = _run(["chain-beds", "--host", "--read-size", str(R), "--merged-in", merged, "--retired-bed", "-", chain], tmp_path)
    assert r.returncode == 0 and r.stdout == want["retired"]


def test_the_golden_cases_hold_what_they_are_there_for():
    g = {c[0]: c for c in GOLDEN}
    assert g["three"][5]["gaps"] == b"cA\t395\t604\ncA\t695\t954\ncA\t1745\t2154\ncB\t895\t1114\n" and g["three"][5]["retired"] == b"cA\t4000\t4099\ncA\t4700\t4999\n"
    assert b"t1\t90\t119\nt1\t119\t140\n" in g["touch"][5]["gaps"]                      # start == previous end: not merged under the strict rule
    assert g["touch"][5]["retired"] == b"t2\t0\t489\nt2\t849\t1189\nt2\t1311\t1999\n"   # [490, 728] + [729, 848]: two regions, no hole; t1 and t3: covered from base 0, bare behind, no row
    assert g["edges"][5]["gaps"] == b"e1\t0\t187\ne1\t882\t999\ntiny\t0\t39\n" and g["edges"][5]["retired"] == b""
    assert g["order"][5]["retired"].startswith(b"aa\t") and g["order"][5]["gaps"].startswith(b"zz\t")      # the retired step has its own slot order
    assert "chain 3 zz 2500" in g["order"][1] and "\n600\nchain 5" in g["order"][1] and g["random"][1].count("\n") < 2600
    t = cc.parse(g["random"][1])
    assert t.n() == 1900 and len(t.names) == 5


CASES = cc.cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_host_twin_equals_the_restatement(case):
    from airlift_amd import capi
    L = capi.load()
    name, t, R, E, M = case
    g, c, r = cc.tap(L.al_dbg_chainreg_host, t, R, E, M)
    assert g == cc.gaps(t, R, E) and c == cc.constant(t) and r == cc.retired(t, M, R)
    g2, c2, r2 = cc.tap(L.al_dbg_chainreg_host, t, R, E, None)
    assert (g2, c2, r2) == (g, c, None)


def test_the_restatement_gives_the_golden_bytes_and_the_cases_reach_their_paths():
    for name, chain, merged, R, E, want in GOLDEN:
        t = cc.parse(chain); M = cc.parse_merged(merged)
        assert cc.bed(cc.gaps(t, R, E), t.names) == want["gaps"] and cc.bed(cc.constant(t), t.names) == want["constant"]
        assert cc.bed(cc.retired(t, M, R), cc.retired_slots(t, M)) == want["retired"]
    by = {c[0]: c for c in CASES}
    for n in cc.SIZES + (cc.BIG,):
        t = by["all_merge_%d" % n][1]
        assert t.n() == n and len(cc.gaps(t, 10, 2)) == (1 if n > 1 else 0)
        assert len(cc.gaps(by["none_merge_%d" % n][1], 10, 0)) == n - 1 and len(cc.retired(by["none_merge_%d" % n][1], [], 10)) == n + 1
    assert len(by["chain_per_line_4097"][1].c_slot) == 4097
    assert cc.gaps(by["single_points"][1], 1, 0) == [(0, 49, 51), (0, 97, 99), (0, 99, 99), (0, 99, 99)]
    a, b = cc.gaps(by["equal_starts_short_first"][1], 90, 10), cc.gaps(by["equal_starts_long_first"][1], 90, 10)
    assert a[0][:2] == b[0][:2] == (0, 0) and len(by["random_%d" % cc.BIG][1].chain) == cc.BIG


def test_the_taps_refuse_a_table_that_breaks_what_the_parser_guarantees():
    from airlift_amd import capi
    L = capi.load()
    for breaker in ("beyond", "size0", "slot"):
        t = cc.Table(); t.header("x", 100, 0); t.line(50, 10); t.line(40)
        if breaker == "beyond": t.size[1] = 41
        if breaker == "size0": t.size[0] = 0
        if breaker == "slot": t.c_slot[0] = 3
        with pytest.raises(AssertionError):
            cc.tap(L.al_dbg_chainreg_host, t, 10, 0, [])


@pytest.mark.parametrize("host", [["--host"], []], ids=["host", "device"])
def test_malformed_chain_files_are_refused_with_file_and_line(host, tmp_path):
    """... before any device is opened: none is visible, and the message does not come from HIP"""
    for k, (text, bad) in enumerate(cc.MALFORMED):
        fn = tmp_path / ("bad%d.chain" % k); fn.write_text(text)
        r = _run(["chain-beds"] + host + ["--read-size", "100", "--max-errors", "5", "--gaps-out", "g.bed", "--constant-bed", "-", str(fn)], tmp_path)
        assert r.returncode == 1 and r.stdout == b"", (text, r.stderr)
        assert ("%s:%d: " % (fn, bad)).encode() in r.stderr and r.stderr.count(b"\n") == 1 and b"HIP" not in r.stderr and b"hip" not in r.stderr, (text, r.stderr)
        assert not os.path.exists(tmp_path / "g.bed")


def test_malformed_merged_beds_are_refused_with_file_and_line(tmp_path):
    chain = tmp_path / "ok.chain"; chain.write_text(cc.HDR + "100\n")
    for k, (text, bad) in enumerate(cc.MERGED_MALFORMED):
        fn = tmp_path / ("bad%d.bed" % k); fn.write_text(text)
        r = _run(["chain-beds", "--read-size", "100", "--merged-in", str(fn), "--retired-bed", "r.bed", str(chain)], tmp_path)
        assert r.returncode == 1 and r.stdout == b"" and ("%s:%d: " % (fn, bad)).encode() in r.stderr and r.stderr.count(b"\n") == 1 and b"HIP" not in r.stderr, (text, r.stderr)
        assert not os.path.exists(tmp_path / "r.bed")
    r = _run(["chain-beds", "--host", "--read-size", "100", "--merged-in", str(tmp_path / "none.bed"), "--retired-bed", "r.bed", str(chain)], tmp_path)
    assert r.returncode == 1 and b"none.bed" in r.stderr and r.stderr.count(b"\n") == 1
    r = _run(["chain-beds", "--host", "--read-size", "100", "--constant-bed", "c.bed", str(tmp_path / "none.chain")], tmp_path)
    assert r.returncode == 1 and b"none.chain" in r.stderr and r.stderr.count(b"\n") == 1 and not os.path.exists(tmp_path / "c.bed")


BAD_ARGS = [(["--read-size", "100", "x.chain"], b"at least one of"), (["--read-size", "100", "--gaps-out", "g.bed", "x.chain"], b"--max-errors"),
            (["--read-size", "100", "--retired-bed", "r.bed", "x.chain"], b"--merged-in"),
            (["--read-size", "100", "--max-errors", "1", "--gaps-out", "-", "--constant-bed", "-", "x.chain"], b"stdout")]


@pytest.mark.parametrize("args,what", BAD_ARGS, ids=[w.decode() for _, w in BAD_ARGS])
def test_chain_beds_refuses_an_incomplete_command_line(args, what, tmp_path):
    r = _run(["chain-beds"] + args, tmp_path)
    assert r.returncode == 1 and r.stdout == b"" and what in r.stderr and r.stderr.count(b"\n") == 1 and b"x.chain" not in r.stderr
    assert not os.listdir(tmp_path)


def test_chain_beds_without_its_arguments_prints_its_usage(tmp_path):
    for args in ([], ["--gaps-out", "g.bed", "x.chain"], ["--read-size", "100", "--constant-bed", "c.bed"]):
        r = _run(["chain-beds"] + args, tmp_path)
        assert r.returncode == 1 and b"Usage: airlift-align chain-beds" in r.stderr


def test_capi_refuses_a_call_without_chain_or_output(tmp_path):
    from airlift_amd import capi
    L = capi.load()
    libc = C.CDLL(None); libc.fopen.restype = C.c_void_p; libc.fopen.argtypes = [C.c_char_p, C.c_char_p]; libc.fclose.argtypes = [C.c_void_p]
    chain = tmp_path / "ok.chain"; chain.write_text(cc.HDR + "100\n")
    out = libc.fopen(str(tmp_path / "o.txt").encode(), b"wb")
    try:
        H = 1    # the C-ABI's flag for the host twin
        assert L.al_chain_beds(str(chain).encode(), 100, 5, None, None, None, None, H, -1) == -1
        assert L.al_chain_beds(None, 100, 5, None, out, None, None, H, -1) == -1
        assert L.al_chain_beds(str(chain).encode(), 0, 5, None, out, None, None, H, -1) == -1
        assert L.al_chain_beds(str(chain).encode(), 100, -1, None, out, None, None, H, -1) == -1
        assert L.al_chain_beds(str(chain).encode(), 100, 5, None, None, None, out, H, -1) == -1
        assert os.path.getsize(tmp_path / "o.txt") == 0
        assert L.al_chain_beds(str(chain).encode(), 100, 5, None, None, out, None, H, -1) == 0
    finally:
        libc.fclose(out)
    assert (tmp_path / "o.txt").read_bytes() == b"cA\t100\t199\n"


# ---- tokens --chain: the command line ----------------------------------------------------------------------------------------------------------------
def _tok(args, tmp_path, files=("ref.fa",), env=None):
    return _run(args + [str(tmp_path / f) for f in files], tmp_path, env)


def _only_the_refusal(r, tmp_path):
    assert r.returncode == 1 and r.stdout == b""
    assert b"failed to open" not in r.stderr and b"HIP" not in r.stderr and b"hip" not in r.stderr and b"Usage" not in r.stderr
    assert not os.listdir(tmp_path)
    assert b"--chain" in r.stderr and r.stderr.count(b"\n") == 1


OTHER_MODE = [["mem"] + CH, ["aln"] + CH, ["samse"] + CH, ["-ax", "sr"] + CH, ["remap"] + CH + ["-o", "o.sam"], ["extract-reads"] + CH, ["extract-sequence"] + CH, ["index"] + CH, ["chain-beds"] + CH]
COMBINED = [(TOK + CH + ["--paf"], b"--paf"), (TOK + ["--bam"] + CH, b"--bam"), (TOK + CH + ["--sorted-bam"], b"--sorted-bam"), (TOK + CH + ["--count-candidates"], b"--count-candidates"),
            (TOK + CH + ["--devices", "0,1"], b"--devices"), (TOK + CH + ["--world", "2", "--rank", "0", "-o", "o.sam"], b"--world"), (TOK + CH + ["--rank", "0"], b"--rank"),
            (TOK + CH + ["--ranked"], b"--ranked"), (TOK + CH + ["--retired-bed", "x.bed", "--paf"], b"--paf"), (TOK + CH + ["--constant-bed", "y.bed", "--bam"], b"--bam")]


@pytest.mark.parametrize("args", OTHER_MODE, ids=[a[0] for a in OTHER_MODE])
def test_cli_refuses_the_option_outside_tokens(args, tmp_path):
    r = _tok(args, tmp_path)
    _only_the_refusal(r, tmp_path)
    assert b"cannot be combined with another mode" in r.stderr


@pytest.mark.parametrize("args,what", COMBINED, ids=[" ".join(a[9:]) for a, _ in COMBINED])
def test_cli_refuses_what_the_option_cannot_serve(args, what, tmp_path):
    r = _tok(args, tmp_path, env=dict(RANK="0", WORLD_SIZE="2"))
    _only_the_refusal(r, tmp_path)
    assert what in r.stderr.split(b"cannot be combined with ")[1]


def test_cli_refuses_a_gaps_bed_a_gap_fasta_or_no_max_errors_beside_the_option(tmp_path):
    r = _tok(TOK + CH + ["--gaps-bed", "gaps.bed"], tmp_path)
    _only_the_refusal(r, tmp_path); assert b"--gaps-bed" in r.stderr
    r = _tok(TOK + CH + ["--merged-bed", "m.bed"], tmp_path, files=("ref.fa", "gaps.fa"))
    _only_the_refusal(r, tmp_path); assert b"gaps.fa" in r.stderr and b"reference alone" in r.stderr
    r = _tok(TOK + ["--chain", "x.chain"], tmp_path)
    _only_the_refusal(r, tmp_path); assert b"--max-errors" in r.stderr
    r = _tok(TOK + CH + ["--retired-bed", "-", "--merged-bed", "-"], tmp_path)
    _only_the_refusal(r, tmp_path); assert b"stdout" in r.stderr
    r = _tok(TOK + CH + ["--gaps-out", "-"], tmp_path)
    _only_the_refusal(r, tmp_path); assert b"stdout" in r.stderr


@pytest.mark.parametrize("opt", ["--retired-bed", "--constant-bed", "--gaps-out"])
def test_cli_refuses_the_chain_outputs_without_the_chain(opt, tmp_path):
    for args, files in ((TOK + [opt, "x.bed"], ("ref.fa", "gaps.fa")), (TOK + ["--gaps-bed", "gaps.bed", opt, "x.bed"], ("ref.fa",))):
        r = _tok(args, tmp_path, files=files)
        _only_the_refusal(r, tmp_path)
        assert opt.encode() in r.stderr and b"needs --chain" in r.stderr


@pytest.mark.parametrize("extra", [[], ["--gaps-out", "g.bed"], ["--retired-bed", "x.bed", "--constant-bed", "-"], ["--regions-bed", "x.bed", "--merged-bed", "-", "-K", "2000"]], ids=["sam", "gaps_out", "retired", "regions"])
def test_an_accepted_command_line_fails_as_tokens_does_with_a_missing_reference(extra, tmp_path):
    r = _tok(TOK + CH + extra, tmp_path)
    assert r.returncode == 1 and b"failed to open file" in r.stderr and b"Usage" not in r.stderr and b"ignored" not in r.stderr and r.stdout == b""
    assert not os.listdir(tmp_path)
    r = _tok(TOK + CH, tmp_path, files=())
    assert r.returncode == 1 and b"Usage" in r.stderr


def test_usage_names_the_options():
    r = subprocess.run([CLI], capture_output=True)
    assert r.returncode == 1
    for w in (b"--chain CHAIN", b"--max-errors E", b"--gaps-out FILE", b"--retired-bed FILE", b"--constant-bed FILE", b"chain-beds --read-size R", b"--merged-in MERGED.bed", b"--host"):
        assert w in r.stderr, w
    assert b"--gaps-bed FILE" in r.stderr and b"upper-case ACGTN" in r.stderr and b"--regions-bed FILE" in r.stderr     # (every earlier line is still there)


_CHILD = """
import ctypes as C, sys
import airlift_amd as A
L = A.load()
idx = L.al_idx_str(10, 15, 1, (C.c_char_p * 1)((b"ACGTTGCA" * 2000)[:12000]), (C.c_char_p * 1)(b"c2"))      # (one contig: c2)
io, mo = A.IdxOpt(), A.MapOpt()
L.al_set_opt(None, C.byref(io), C.byref(mo)); L.al_set_opt(b"sr", C.byref(io), C.byref(mo))
libc = C.CDLL(None); libc.fopen.restype = C.c_void_p; libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
out = libc.fopen(sys.argv[2].encode(), b"wb")
if sys.argv[3] == "regions":
    print(L.al_map_tokens_chain_regions(idx, sys.argv[1].encode(), int(sys.argv[4]), 100, 7, C.byref(mo), 1, out, None, -1, None, None, None))
else:
    print(L.al_map_tokens_chain_file(idx, sys.argv[1].encode(), int(sys.argv[4]), 100, 7, C.byref(mo), 1, out, None, -1, None))
"""


@pytest.mark.parametrize("which", ["file", "regions"])
def test_the_capi_refuses_a_malformed_chain_file_and_a_contig_the_index_lacks(which, tmp_path):
    """In a child process (the message is on the C library's stderr): -1, FILE:LINE: in the one message, no device touched (none is visible), nothing written."""
    script = tmp_path / "child.py"; script.write_text(_CHILD)
    env = dict(os.environ, PYTHONPATH=ROOT, **NO_GPU)
    bad = [(t, l, "5") for t, l in cc.MALFORMED[:4]] + [("chain 1 c2 12000 + 0 100 q 9 + 0 100 1\n100\n\nchain 1 cZ 8000 + 0 100 q 9 + 0 100 2\n100\n", 4, "5"), (cc.HDR + "100\n", None, "-1")]
    for k, (text, line, E) in enumerate(bad):
        fn = tmp_path / ("bad%d.chain" % k); fn.write_text(text)
        r = subprocess.run([os.sys.executable, str(script), str(fn), str(tmp_path / "o.txt"), which, E], capture_output=True, env=env, timeout=60)
        assert r.returncode == 0 and r.stdout.strip() == b"-1", (text, r.stderr[-500:])
        assert r.stderr.count(b"\n") == 1 and b"HIP" not in r.stderr and (line is None or ("%s:%d: " % (fn, line)).encode() in r.stderr), (text, r.stderr)
        assert os.path.getsize(tmp_path / "o.txt") == 0

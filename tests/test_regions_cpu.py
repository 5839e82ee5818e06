"""tokens --regions-bed / --merged-bed without a GPU: the command line.  The combinations the regions mode cannot serve exit 1 with a message before the
reference is read or a device opened; an accepted command line gets as far as `tokens` gets today; the C-ABI refuses a call without an output."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
TOK = ["tokens", "--read-size", "100", "--skip", "50"]

OTHER_MODE = [["mem", "--regions-bed", "x.bed"], ["aln", "--merged-bed", "x.bed"], ["samse", "--regions-bed", "x.bed"], ["-ax", "sr", "--merged-bed", "x.bed"],
              ["-ax", "sr", "--regions-bed", "-"], ["remap", "--regions-bed", "x.bed", "-o", "o.sam"], ["extract-reads", "--merged-bed", "x.bed"],
              ["extract-sequence", "--regions-bed", "x.bed"], ["index", "--merged-bed", "x.bed"]]
COMBINED = [(TOK + ["--regions-bed", "x.bed", "--paf"], b"--paf"), (TOK + ["--bam", "--merged-bed", "x.bed"], b"--bam"),
            (TOK + ["--regions-bed", "x.bed", "--sorted-bam"], b"--sorted-bam"), (TOK + ["--merged-bed", "x.bed", "--count-candidates"], b"--count-candidates"),
            (TOK + ["--regions-bed", "x.bed", "--devices", "0,1"], b"--devices"), (TOK + ["--regions-bed", "x.bed", "--devices", "0,0"], b"--devices"),
            (TOK + ["--merged-bed", "x.bed", "--world", "2", "--rank", "0", "-o", "o.sam"], b"--world"), (TOK + ["--merged-bed", "x.bed", "--rank", "0"], b"--rank"),
            (TOK + ["--regions-bed", "x.bed", "--merged-bed", "y.bed", "--ranked"], b"--ranked")]


def _run(args, tmp_path, env=None):
    e = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    e.update(env or {})
    return subprocess.run([CLI] + args + [str(tmp_path / "ref.fa"), str(tmp_path / "gaps.fa")], capture_output=True, env=e, timeout=60, cwd=str(tmp_path))


def _only_the_refusal(r, tmp_path):
    assert r.returncode == 1 and r.stdout == b""
    assert b"failed to open" not in r.stderr and b"HIP" not in r.stderr and b"hip" not in r.stderr and b"Usage" not in r.stderr
    assert not os.path.exists(tmp_path / "x.bed") and not os.path.exists(tmp_path / "y.bed")


@pytest.mark.parametrize("args", OTHER_MODE, ids=[" ".join(a) for a in OTHER_MODE])
def test_cli_refuses_the_options_outside_tokens(args, tmp_path):
    r = _run(args, tmp_path)
    _only_the_refusal(r, tmp_path)
    opt = [a for a in args if a in ("--regions-bed", "--merged-bed")][0].encode()
    assert opt in r.stderr and b"cannot be combined with another mode" in r.stderr


@pytest.mark.parametrize("args,what", COMBINED, ids=[" ".join(a[5:]) for a, _ in COMBINED])
def test_cli_refuses_what_the_regions_mode_cannot_serve(args, what, tmp_path):
    r = _run(args, tmp_path, env=dict(RANK="0", WORLD_SIZE="2"))
    _only_the_refusal(r, tmp_path)
    assert b"--regions-bed / --merged-bed" in r.stderr and what in r.stderr.split(b"cannot be combined with ")[1]


def test_cli_refuses_two_outputs_on_stdout(tmp_path):
    r = _run(TOK + ["--regions-bed", "-", "--merged-bed", "-"], tmp_path)
    _only_the_refusal(r, tmp_path)
    assert b"at most one of them may be '-'" in r.stderr


@pytest.mark.parametrize("extra", [[], ["--MD"], ["--cs", "--eqx", "-Y", "--secondary=yes"]], ids=["plain", "MD", "cs_eqx_Y_secondary"])
def test_an_accepted_command_line_fails_as_tokens_does_with_a_missing_reference(extra, tmp_path):
    """Options and their FILEs are read (none becomes a positional argument: no usage text, no 'ignored'), and the run ends where `tokens` ends today."""
    today = _run(TOK + extra, tmp_path)
    r = _run(TOK + extra + ["--regions-bed", "x.bed", "--merged-bed", "-"], tmp_path)
    assert today.returncode == 1 and b"failed to open file" in today.stderr
    assert (r.returncode, r.stdout, r.stderr) == (today.returncode, today.stdout, today.stderr)
    assert b"Usage" not in r.stderr and b"ignored" not in r.stderr
    assert not os.path.exists(tmp_path / "x.bed")


def test_usage_names_the_options():
    r = subprocess.run([CLI], capture_output=True)
    assert r.returncode == 1 and b"--regions-bed FILE" in r.stderr and b"--merged-bed FILE" in r.stderr


def test_capi_refuses_a_call_without_an_output():
    import airlift_amd as A
    L = A.load()
    idx = L.al_idx_str(10, 15, 1, (C.c_char_p * 1)(b"ACGT" * 500), (C.c_char_p * 1)(b"c"))
    assert idx
    io, mo = A.IdxOpt(), A.MapOpt()
    L.al_set_opt(None, C.byref(io), C.byref(mo)); L.al_set_opt(b"sr", C.byref(io), C.byref(mo))
    try:
        assert L.al_map_tokens_regions(idx, b"/nonexistent/gaps.fa", 100, 50, C.byref(mo), 1, None, None, -1) == -1
    finally:
        L.al_idx_destroy(idx)

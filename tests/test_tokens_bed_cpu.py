"""tokens --gaps-bed without a GPU: the command line and the C-ABI's argument checks.  What the option cannot be combined with exits 1 with a message that
names it, before the reference is read or a device opened; an accepted command line gets as far as `tokens` gets today; the two C-ABI calls refuse a call
without a BED or an output, and a malformed row with its file and line number -- the BED is read against the index before any device is opened."""
import ctypes as C
import os
import subprocess

import pytest

import tokens_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
TOK = ["tokens", "--read-size", "100", "--skip", "50"]
GB = ["--gaps-bed", "gaps.bed"]

OTHER_MODE = [["mem"] + GB, ["aln"] + GB, ["samse"] + GB, ["-ax", "sr"] + GB, ["remap"] + GB + ["-o", "o.sam"], ["extract-reads"] + GB, ["extract-sequence"] + GB, ["index"] + GB]
COMBINED = [(TOK + GB + ["--paf"], b"--paf"), (TOK + ["--bam"] + GB, b"--bam"), (TOK + GB + ["--sorted-bam"], b"--sorted-bam"), (TOK + GB + ["--count-candidates"], b"--count-candidates"),
            (TOK + GB + ["--devices", "0,1"], b"--devices"), (TOK + GB + ["--devices", "0,0"], b"--devices"), (TOK + GB + ["--world", "2", "--rank", "0", "-o", "o.sam"], b"--world"),
            (TOK + GB + ["--rank", "0"], b"--rank"), (TOK + GB + ["--ranked"], b"--ranked"),
            (TOK + GB + ["--regions-bed", "x.bed", "--paf"], b"--paf"), (TOK + GB + ["--merged-bed", "y.bed", "--bam"], b"--bam"), (TOK + GB + ["--regions-bed", "x.bed", "--devices", "0-1"], b"--devices")]


def _run(args, tmp_path, files=("ref.fa",), env=None):
    e = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    e.update(env or {})
    return subprocess.run([CLI] + args + [str(tmp_path / f) for f in files], capture_output=True, env=e, timeout=60, cwd=str(tmp_path))


def _only_the_refusal(r, tmp_path):
    assert r.returncode == 1 and r.stdout == b""
    assert b"failed to open" not in r.stderr and b"HIP" not in r.stderr and b"hip" not in r.stderr and b"Usage" not in r.stderr
    assert not os.path.exists(tmp_path / "x.bed") and not os.path.exists(tmp_path / "y.bed")
    assert b"--gaps-bed" in r.stderr and r.stderr.count(b"\n") == 1


@pytest.mark.parametrize("args", OTHER_MODE, ids=[" ".join(a) for a in OTHER_MODE])
def test_cli_refuses_the_option_outside_tokens(args, tmp_path):
    r = _run(args, tmp_path)
    _only_the_refusal(r, tmp_path)
    assert b"cannot be combined with another mode" in r.stderr


@pytest.mark.parametrize("args,what", COMBINED, ids=[" ".join(a[5:]) for a, _ in COMBINED])
def test_cli_refuses_what_the_option_cannot_serve(args, what, tmp_path):
    r = _run(args, tmp_path, env=dict(RANK="0", WORLD_SIZE="2"))
    _only_the_refusal(r, tmp_path)
    assert what in r.stderr.split(b"cannot be combined with ")[1]


@pytest.mark.parametrize("extra", [[], ["--regions-bed", "x.bed"], ["--merged-bed", "-"]], ids=["sam", "regions", "merged"])
def test_cli_refuses_a_gap_fasta_beside_the_option(extra, tmp_path):
    r = _run(TOK + GB + extra, tmp_path, files=("ref.fa", "gaps.fa"))
    _only_the_refusal(r, tmp_path)
    assert b"gaps.fa" in r.stderr and b"reference alone" in r.stderr


@pytest.mark.parametrize("extra", [[], ["--MD"], ["--secondary=yes", "-K", "2000"], ["--regions-bed", "x.bed", "--merged-bed", "-"]], ids=["plain", "MD", "secondary_K", "regions"])
def test_an_accepted_command_line_fails_as_tokens_does_with_a_missing_reference(extra, tmp_path):
    """The option and its FILE are read (neither becomes a positional argument: no usage text, no 'ignored'), and the run ends where `tokens` ends today."""
    today = _run(TOK + extra, tmp_path, files=("ref.fa", "gaps.fa"))
    r = _run(TOK + extra + GB, tmp_path)
    assert today.returncode == 1 and b"failed to open file" in today.stderr
    assert (r.returncode, r.stdout, r.stderr) == (today.returncode, today.stdout, today.stderr)
    assert b"Usage" not in r.stderr and b"ignored" not in r.stderr
    assert not os.path.exists(tmp_path / "x.bed")
    # without a reference at all: the usage text, as `tokens` without its files
    r = _run(TOK + GB, tmp_path, files=())
    assert r.returncode == 1 and b"Usage" in r.stderr


def test_usage_names_the_option():
    r = subprocess.run([CLI], capture_output=True)
    assert r.returncode == 1 and b"--gaps-bed FILE" in r.stderr and b"upper-case ACGTN" in r.stderr


@pytest.fixture(scope="module")
def lib_idx():
    import airlift_amd as A
    L = A.load()
    names = [n for n, _ in tc.CONTIGS]; seqs = [(b"ACGTTGCA" * 2000)[:l] for _, l in tc.CONTIGS]
    idx = L.al_idx_str(10, 15, 1, (C.c_char_p * 3)(*seqs), (C.c_char_p * 3)(*names))
    assert idx
    io, mo = A.IdxOpt(), A.MapOpt()
    L.al_set_opt(None, C.byref(io), C.byref(mo)); L.al_set_opt(b"sr", C.byref(io), C.byref(mo))
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p; libc.fopen.argtypes = [C.c_char_p, C.c_char_p]; libc.fclose.argtypes = [C.c_void_p]
    yield L, idx, mo, libc
    L.al_idx_destroy(idx)


def test_capi_refuses_a_call_without_bed_or_output(lib_idx, tmp_path):
    L, idx, mo, libc = lib_idx
    bed = tmp_path / "gaps.bed"; bed.write_bytes(b"c2\t1\t300\n")
    out = libc.fopen(str(tmp_path / "o.txt").encode(), b"wb")
    try:
        assert L.al_map_tokens_bed_regions(idx, str(bed).encode(), 100, 50, C.byref(mo), 1, None, None, -1) == -1
        assert L.al_map_tokens_bed_regions(idx, None, 100, 50, C.byref(mo), 1, out, None, -1) == -1
        assert L.al_map_tokens_bed_regions(idx, b"/nonexistent/gaps.bed", 100, 50, C.byref(mo), 1, out, out, -1) == -1
        assert L.al_map_tokens_bed_file(idx, str(bed).encode(), 100, 50, C.byref(mo), 1, None, None, -1) == -1
        assert L.al_map_tokens_bed_file(idx, None, 100, 50, C.byref(mo), 1, out, None, -1) == -1
        assert L.al_map_tokens_bed_file(idx, b"/nonexistent/gaps.bed", 100, 50, C.byref(mo), 1, out, None, -1) == -1
        assert L.al_map_tokens_bed_file(idx, str(bed).encode(), 0, 50, C.byref(mo), 1, out, None, -1) == -1
        assert L.al_map_tokens_bed_regions(idx, str(bed).encode(), 100, 0, C.byref(mo), 1, out, None, -1) == -1
    finally:
        libc.fclose(out)
    assert os.path.getsize(tmp_path / "o.txt") == 0


_CHILD = """
import ctypes as C, sys
import airlift_amd as A
L = A.load()
names = [b"c2", b"cA", b"c10"]; lens = [12000, 8000, 9000]
idx = L.al_idx_str(10, 15, 1, (C.c_char_p * 3)(*[(b"ACGTTGCA" * 2000)[:l] for l in lens]), (C.c_char_p * 3)(*names))
io, mo = A.IdxOpt(), A.MapOpt()
L.al_set_opt(None, C.byref(io), C.byref(mo)); L.al_set_opt(b"sr", C.byref(io), C.byref(mo))
libc = C.CDLL(None); libc.fopen.restype = C.c_void_p; libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
out = libc.fopen(sys.argv[2].encode(), b"wb")
f = L.al_map_tokens_bed_regions if sys.argv[3] == "regions" else L.al_map_tokens_bed_file
print(f(idx, sys.argv[1].encode(), 100, 7, C.byref(mo), 1, out, None, -1))
"""


@pytest.mark.parametrize("which", ["file", "regions"])
def test_malformed_rows_are_refused_with_file_and_line(which, tmp_path):
    """In a child process (the message is on the C library's stderr), every malformed BED of tokens_cases.MALFORMED: -1, `FILE:LINE:` in the one message, no
    device touched (none is visible), nothing written."""
    script = tmp_path / "child.py"; script.write_text(_CHILD)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", PYTHONPATH=ROOT)
    for k, (text, bad) in enumerate(tc.MALFORMED if which == "file" else tc.MALFORMED[:3]):
        bed = tmp_path / ("bad%d.bed" % k); bed.write_bytes(text)
        r = subprocess.run([os.sys.executable, str(script), str(bed), str(tmp_path / "o.txt"), which], capture_output=True, env=env, timeout=60)
        assert r.returncode == 0 and r.stdout.strip() == b"-1", (text, r.stderr[-500:])
        assert ("%s:%d: " % (bed, bad)).encode() in r.stderr and r.stderr.count(b"\n") == 1 and b"HIP" not in r.stderr, (text, r.stderr)
        assert os.path.getsize(tmp_path / "o.txt") == 0

"""extract-sequence --gpu-select=host: the selector's driver (pieces, carry, hand-over) with the kernels' host twin as the backend, no device.  The three
output files are those of the same build's default extract-sequence on every case of select_cases.py, whatever the piece size, plain and BGZF; the
timing line shows that the records went through the selector and not, quietly, through the default reader."""
import os
import re
import subprocess
import sys

import pytest

import select_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
OUT = ("reads_1.fastq", "reads_2.fastq", "singletons.fastq")
CASES = sc.cases()
FIRST_IRREGULAR = {"multiline": 6, "seq_at": 6, "seq_plus": 6, "seq_gt": 6, "fasta": 0}      # file 1's first irregular record (a FASTA file: both files')
LINE = re.compile(r"--gpu-select '([^']*)' \(([^)]*)\): (\d+) pieces, (\d+) bytes in, (\d+) records tested, (\d+) selected, (\d+) handed to the default reader")


def run(args, out_dir, **env):
    os.makedirs(out_dir, exist_ok=True)
    r = subprocess.run([CLI, "extract-sequence"] + args + [str(out_dir)], capture_output=True, env=dict(os.environ, **{k: str(v) for k, v in env.items()}))
    return r, tuple(open(os.path.join(out_dir, f), "rb").read() if os.path.exists(os.path.join(out_dir, f)) else None for f in OUT)


def timing(stderr):
    return [(m.group(2), int(m.group(3)), int(m.group(4)), int(m.group(5)), int(m.group(6)), int(m.group(7))) for m in LINE.finditer(stderr.decode())]


def n_records(text):
    """Records of a regular four-line text (an unterminated last line counts)."""
    return (text.count(b"\n") + (0 if text.endswith(b"\n") else 1)) // 4


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Every case written once, with the default extract-sequence's output as the reference of all tests of this module."""
    d = tmp_path_factory.mktemp("select")
    out = {}
    for c in CASES:
        p = d / c.name; p.mkdir()
        fq = [str(p / "r1.fq"), str(p / "r2.fq")]; rows = str(p / "rows.bed")
        for f, t in zip(fq, c.fq):
            open(f, "wb").write(t)
        open(rows, "wb").write(sc.rows(c.l1, c.l2))
        r, exp = run(fq + [rows], p / "default")
        assert r.returncode == 0, r.stderr.decode()
        out[c.name] = dict(fq=fq, rows=rows, exp=exp, dir=p)
    return out


@pytest.mark.parametrize("piece", [512, 1000, 4096, None])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_output_equals_the_default_reader(files, case, piece):
    f = files[case.name]
    r, got = run(["--gpu-select=host"] + (["--select-piece", str(piece)] if piece else []) + f["fq"] + [f["rows"]], f["dir"] / ("p%s" % piece), AL_TIMING=1)
    assert r.returncode == 0, r.stderr.decode()
    assert got == f["exp"]
    if case.name in ("base", "all"):
        assert got[0].count(b"\n") >= 4 * 30
    t = timing(r.stderr)
    assert len(t) == 2 and all(x[0] == "host twin" for x in t), r.stderr.decode()
    for k in (0, 1):
        backend, pieces, bytes_in, tested, selected, handed = t[k]
        assert handed == case.handed[k], (k, t[k])
        irregular = (case.name in FIRST_IRREGULAR and k == 0) or case.name == "fasta"
        assert tested == (FIRST_IRREGULAR[case.name] if irregular else n_records(case.fq[k]) if case.name != "trailing_blank" or k else 12), (k, t[k])
        assert bytes_in >= len(case.fq[k]) or irregular
        if piece and piece < len(case.fq[k]) // 2 and case.handed[k] == 0:
            assert pieces > 1


@pytest.mark.parametrize("case", [c for c in CASES if c.oracle], ids=[c.name for c in CASES if c.oracle])
def test_plain_cases_equal_the_oracle(files, case):
    import n1_oracle as o
    f = files[case.name]
    r, got = run(["--gpu-select=host", "--select-piece", "1000"] + f["fq"] + [f["rows"]], f["dir"] / "oracle")
    assert r.returncode == 0
    assert got == o.extract_sequence(f["fq"][0], f["fq"][1], sc.rows(case.l1, case.l2).decode().split("\n")[:-1])


@pytest.fixture(scope="module")
def bgzf_files(files, tmp_path_factory):
    d = tmp_path_factory.mktemp("select_bgzf")
    out = {}
    for name in ("base", "multiline", "unterminated"):
        c = [x for x in CASES if x.name == name][0]
        for block in (700, 0xff00):
            p = [str(d / ("%s_%d_%d.fq.gz" % (name, block, k))) for k in (1, 2)]
            for f, t in zip(p, c.fq):
                open(f, "wb").write(sc.bgzf(t, block))
            out[name, block] = p
    return out


@pytest.mark.parametrize("name,block,piece_kb,piece,mixed", [("base", 700, 1, 512, False), ("base", 700, 3, 4096, False), ("base", 0xff00, 16, 1000, False), ("base", 0xff00, None, None, False),
                                                           ("base", 700, 2, 4096, True), ("multiline", 700, 1, 512, False), ("unterminated", 0xff00, 4, 1000, True)])
def test_bgzf_input_with_gpu_inflate(files, bgzf_files, name, block, piece_kb, piece, mixed):
    f = files[name]; z = bgzf_files[name, block]; case = [x for x in CASES if x.name == name][0]
    fq = [f["fq"][0], z[1]] if mixed else z
    env = dict(AL_TIMING=1); env.update({"AL_INFLATE_PIECE_KB": piece_kb} if piece_kb else {})
    r, got = run(["--gpu-select=host", "--gpu-inflate"] + (["--select-piece", str(piece)] if piece else []) + fq + [f["rows"]], f["dir"] / ("z%d_%s_%s" % (block, piece_kb, mixed)), **env)
    assert r.returncode == 0, r.stderr.decode()
    assert got == f["exp"]
    t = timing(r.stderr)
    assert len(t) == 2 and [x[5] for x in t] == list(case.handed) and all(x[3] > 0 for x in t)
    assert b"is read as one gzip stream" not in r.stderr


def test_bgzf_without_gpu_inflate_and_plain_gzip_take_the_default_reader_with_a_notice(files, bgzf_files, tmp_path):
    import gzip
    f = files["base"]
    r, got = run(["--gpu-select=host"] + bgzf_files["base", 700] + [f["rows"]], tmp_path / "a")
    assert r.returncode == 0 and got == f["exp"] and r.stderr.count(b"is read as one gzip stream on the host") == 2
    gz = str(tmp_path / "r1.fq.gz"); open(gz, "wb").write(gzip.compress(open(f["fq"][0], "rb").read()))
    r, got = run(["--gpu-select=host", "--gpu-inflate", gz, f["fq"][1], f["rows"]], tmp_path / "b", AL_TIMING=1)
    assert r.returncode == 0 and got == f["exp"] and r.stderr.count(b"is not a BGZF file; it is read as one gzip stream on the host") == 1
    assert len(timing(r.stderr)) == 1


def test_damaged_bgzf_input_is_an_error_that_names_the_offset(files, tmp_path):
    f = files["base"]; c = [x for x in CASES if x.name == "base"][0]
    whole = sc.bgzf(c.fq[0], 20000)
    cut = str(tmp_path / "cut.fq.gz"); open(cut, "wb").write(whole[:len(whole) - 28 - 100])
    r, _ = run(["--gpu-select=host", "--gpu-inflate", cut, f["fq"][1], f["rows"]], tmp_path / "a")
    assert r.returncode == 1 and b"truncated BGZF member at file offset" in r.stderr
    k = len(sc.bgzf(c.fq[0][:20000], 20000, eof=False)); k2 = k + len(sc.bgzf(c.fq[0][20000:40000], 20000, eof=False))
    crc = str(tmp_path / "crc.fq.gz"); open(crc, "wb").write(whole[:k2 - 8] + bytes([whole[k2 - 8] ^ 1]) + whole[k2 - 7:])
    r, _ = run(["--gpu-select=host", "--gpu-inflate", f["fq"][1], crc, f["rows"]], tmp_path / "b")
    assert r.returncode == 1 and ("BGZF member at file offset %d: status 10" % k).encode() in r.stderr


def test_the_four_positional_form_still_runs_and_tolerates_trailing_arguments(files, tmp_path):
    f = files["base"]
    r, got = run(f["fq"] + [f["rows"]], tmp_path / "x")
    assert r.returncode == 0 and got == f["exp"]
    os.makedirs(tmp_path / "y")
    r = subprocess.run([CLI, "extract-sequence"] + f["fq"] + [f["rows"], str(tmp_path / "y"), "4", "extra"], capture_output=True)
    assert r.returncode == 0 and open(tmp_path / "y" / OUT[0], "rb").read() == f["exp"][0]


def test_the_library_entry_takes_the_flags(files, tmp_path):
    code = ("import ctypes as C, sys\nfrom airlift_amd import capi\nL = capi.load()\nnp, ns = C.c_int64(0), C.c_int64(0)\n"
            "print(L.al_extract_sequence_ex(sys.argv[1].encode(), sys.argv[2].encode(), sys.argv[3].encode(), sys.argv[4].encode(), C.byref(np), C.byref(ns), 2 | 4, -1, 1, 777), np.value, ns.value)\n")
    f = files["base"]; os.makedirs(tmp_path / "o")
    r = subprocess.run([sys.executable, "-c", code] + f["fq"] + [f["rows"], str(tmp_path / "o")], capture_output=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()
    rc, n_pairs, n_single = (int(x) for x in r.stdout.split())
    assert rc == 0 and n_pairs == f["exp"][0].count(b"\n") // 4 and n_single == f["exp"][2].count(b"\n") // 4
    assert tuple(open(tmp_path / "o" / x, "rb").read() for x in OUT) == f["exp"]

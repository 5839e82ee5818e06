"""-m gpu tests of `airlift-align bam-index`, every GPU step under a time limit of its own (the command through run_index, the taps and the C ABI in a child
process, tests/helpers/index_child.py): the kernels against their host twin and against the rules restated in Python (index_cases.py) through the taps over the
case lists and the piece sizes; the command on the device against `--host` byte for byte over member size and piece size; the refusals on the device path; the C
ABI; merge --write-index on the device, without and with --gpu-deflate, against `bam-index --host` of its output."""
import os
import subprocess
import sys

import pytest

import index_cases as ic
import merge_cases as mc
from select_cases import bgzf
from test_index_cpu import cli_end, piece_args, refused, run_cmd, run_index, write_case

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "helpers", "index_child.py")


def run_child(what, d, limit=120):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, CHILD, what, str(d)], capture_output=True)
    assert r.returncode == 0, "[%s] exit status %d\n%s\n%s" % (what, r.returncode, r.stdout.decode()[-2000:], r.stderr.decode()[-3000:])
    assert r.stdout.decode().strip().split("\n")[-1].startswith("ok " + what)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("gpu_index"), ic.all_cases()


def test_the_taps_equal_their_host_twin_and_python(work):
    run_child("taps", work[0])


def test_the_taps_refuse_what_the_twin_refuses(work):
    run_child("refusals", work[0])


def test_the_c_abi_on_the_device(work):
    run_child("abi", work[0])


@pytest.mark.parametrize("piece", [1000, 4096, None])
@pytest.mark.parametrize("block", ic.BLOCKS)
def test_the_command_on_the_device_equals_host_and_python(work, block, piece):
    d, cases = work
    pa, kb = piece_args(piece)
    names = ["%s@%d" % (n, block) for n in ("boundaries", "basics", "one_bin", "n65", "header_only")] + (sorted(ic.cut_cases()) if block == 700 else [])
    for name in names:
        recs, layout = cases[name]
        bam, data = write_case(d, name, recs, layout)
        rh, target = run_index(bam, *pa, **kb)
        assert rh.returncode == 0, rh.stderr.decode()[-1500:]
        host = open(target, "rb").read()
        r, target = run_index(bam, *pa, host=False, AL_TIMING=1, **kb)
        assert r.returncode == 0, (name, r.stderr.decode()[-1500:])
        got = open(target, "rb").read()
        assert got == host and got == ic.expected_bai(ic.REFS, recs, ic.members(data)), (name, block, piece)
        err = r.stderr.decode()
        assert "(k_bai):" in err and "device bytes held at return: 0\n" in err and "the host twin builds" not in err, err[-1500:]


@pytest.mark.parametrize("name", sorted(ic.refusals()))
def test_input_without_an_index_is_refused_on_the_device(tmp_path, name):
    recs, say = ic.refusals()[name]
    bam = str(tmp_path / (name + ".bam")); open(bam, "wb").write(bgzf(ic.stream(recs), 700))
    r, target = run_index(bam, "--piece", "1000", host=False, AL_INFLATE_PIECE_KB=2)
    refused(r, target, "ERROR: '%s': " % bam + say)


@pytest.mark.parametrize("piece", ic.PIECES)
def test_a_descent_across_a_piece_boundary_is_refused_on_the_device(tmp_path, piece):
    recs, off = ic.boundary_descent(cli_end(piece))
    bam = str(tmp_path / "boundary.bam"); open(bam, "wb").write(bgzf(ic.stream(recs), 700))
    r, target = run_index(bam, "--piece", str(piece), host=False, AL_INFLATE_PIECE_KB=2)
    refused(r, target, "ERROR: '%s': not in coordinate order at offset %d of the inflated stream" % (bam, off))


@pytest.mark.parametrize("name", sorted(mc.malformed()))
def test_malformed_input_is_refused_on_the_device(tmp_path, name):
    _, blob, say = mc.malformed()[name]
    bam = str(tmp_path / "bad.bam"); open(bam, "wb").write(bgzf(blob, 700))
    r, target = run_index(bam, "--piece", "1000", host=False, AL_INFLATE_PIECE_KB=1)
    refused(r, target, "ERROR: '%s': malformed BAM record at " % bam + say)


@pytest.mark.parametrize("deflate", [False, True])
def test_merge_write_index_on_the_device(tmp_path, deflate):
    inputs = mc.windows(1000)["k3"]
    bams = []
    for i, x in enumerate(inputs):
        bams.append(str(tmp_path / ("in%d.bam" % i))); open(bams[-1], "wb").write(bgzf(mc.stream(x), 700))
    out = str(tmp_path / "merged.bam")
    r = run_cmd(["merge", "--write-index", "-o", out, "--piece", "1000"] + (["--gpu-deflate"] if deflate else []) + bams, AL_INFLATE_PIECE_KB=2, AL_TIMING=1)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-1500:]
    assert "(k_merge):" in err and "[airlift] bam-index: '%s' into '%s.bai' (k_bai):" % (out, out) in err and err.count("device bytes held at return: 0\n") == 2, err[-1500:]
    got = open(out + ".bai", "rb").read()
    rh, target = run_index(out)
    assert rh.returncode == 0 and open(target, "rb").read() == got
    contigs, no_coor = ic.parse_bai(got)
    assert contigs[0]["pseudo"][2] == sum(len(i[2]) for i in inputs) and no_coor == 0

"""-m gpu tests of `airlift-align lift --sorted`, every GPU step under a time limit of its own (the command through run_lift, the taps and the C ABI in a
child process, tests/helpers/lift_sort_child.py): the compaction, the descent count, the sort and the permuted gather against their host twin and against
the rules restated in Python (lift_sort_cases.py) through the taps; the command on the device against `--host --sorted`, Python and the flagless run over
member size, piece size, --gpu-deflate and --sort-mem; the C ABI; the malformed inputs."""
import os
import subprocess
import sys

import pytest

import lift_cases as lc
import lift_sort_cases as ls
from select_cases import bgzf
from test_lift_cpu import MALFORMED, run_lift
from test_lift_sorted_cpu import check_sorted, timing

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "helpers", "lift_sort_child.py")


def run_child(what, d, limit=120):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, CHILD, what, str(d)], capture_output=True)
    assert r.returncode == 0, "[%s] exit status %d\n%s\n%s" % (what, r.returncode, r.stdout.decode()[-2000:], r.stderr.decode()[-3000:])
    assert r.stdout.decode().strip().split("\n")[-1].startswith("ok " + what)


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    from airlift_amd import capi
    L = capi.load()
    d = tmp_path_factory.mktemp("gpu_lift_sorted")
    chain = str(d / "directed.chain"); open(chain, "w").write(lc.CHAIN)
    return L, d, chain, L.al_dbg_lift_window()             # (a constant of the library: no GPU step)


def test_the_taps_equal_their_host_twin_and_python(env):
    run_child("taps", env[1])


def test_the_order_is_made_on_the_host_when_the_temporaries_are_refused(env):
    run_child("fallback", env[1])


def test_the_c_abi_with_the_sorted_flag(env):
    run_child("abi", env[1])


@pytest.fixture(scope="module")
def cli_case(env):
    """the matrix's input at both member sizes; per member size the flagless run and, per piece size and --sort-mem, the `--host --sorted` run"""
    L, d, chain, W = env
    recs = lc.directed(257) + lc.walk_sets(W)["long"] + lc.walk_sets(W)["cut1"]
    out = {}
    for block in (700, 0xff00):
        bam = str(d / ("cli%d.bam" % block)); open(bam, "wb").write(bgzf(lc.bam_bytes(lc.HEADER, lc.REFS, recs), block))
        fd = d / ("flagless%d" % block); fd.mkdir()
        r, o, b = run_lift(fd, bam, chain, "--piece", "4096", AL_INFLATE_PIECE_KB=2)
        assert r.returncode == 0, r.stderr.decode()[-1500:]
        out[block] = (bam, o, b)
    return recs, out, {}


@pytest.mark.parametrize("sort_mem", [2000, None])
@pytest.mark.parametrize("deflate", [False, True])
@pytest.mark.parametrize("piece", [1000, 4096, None])
@pytest.mark.parametrize("block", [700, 0xff00])
def test_lift_sorted_on_the_device_equals_host_python_and_the_flagless_records(env, cli_case, tmp_path, block, piece, deflate, sort_mem):
    L, d, chain, W = env
    recs, case, host_runs = cli_case
    bam, fo, fb = case[block]
    common = ["--sorted"] + (["--piece", str(piece)] if piece else []) + (["--sort-mem", str(sort_mem)] if sort_mem else [])
    kb = dict(AL_INFLATE_PIECE_KB=2 if piece else 1024, AL_TIMING=1)
    if (block, piece, sort_mem) not in host_runs:
        hd = d / ("host_%d_%s_%s" % (block, piece, sort_mem)); hd.mkdir()
        rh, out_h, bed_h = run_lift(hd, bam, chain, *common, **kb)
        assert rh.returncode == 0 and "(host twin):" in rh.stderr.decode(), rh.stderr.decode()[-1500:]
        host_runs[block, piece, sort_mem] = (ls.inflate(out_h), open(bed_h, "rb").read())
    host_stream, host_bed = host_runs[block, piece, sort_mem]
    r, out, bed = run_lift(tmp_path, bam, chain, *common, *(["--gpu-deflate"] if deflate else []), host=False, **kb)
    stream = check_sorted(r, out, bed, lc.HEADER, lc.REFS, recs, lc.CHAIN, (fo, fb))
    assert stream == host_stream and open(bed, "rb").read() == host_bed
    err = r.stderr.decode()
    assert "(k_lift):" in err and "device bytes held at return: 0\n" in err and "the host twin lifts" not in err and "sorted on the host" not in err, err[-1500:]
    assert timing(err, "pieces in order") + timing(err, "pieces sorted") == timing(err, "pieces,") and timing(err, "pieces sorted") >= 1
    if sort_mem and piece:
        assert timing(err, "spills") >= 2
    if not sort_mem:
        assert timing(err, "spills") == 0
    if deflate:
        assert "BAM output: deflate (device" in err, err[-1500:]


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_input_is_refused_as_without_the_flag(env, tmp_path, name):
    L, d, chain, W = env
    blob, say = MALFORMED[name]
    bam = str(tmp_path / "bad.bam"); open(bam, "wb").write(bgzf(blob, 700))
    res = []
    for extra in ([], ["--sorted"]):
        r, out, bed = run_lift(tmp_path, bam, chain, "--piece", "1000", *extra, host=False, AL_INFLATE_PIECE_KB=1)
        assert r.returncode == 1 and say in r.stderr.decode() and not os.path.exists(out) and not os.path.exists(bed), r.stderr.decode()[-800:]
        res.append([l for l in r.stderr.decode().split("\n") if l.startswith("ERROR")])
    assert res[0] == res[1] and len(res[0]) == 1

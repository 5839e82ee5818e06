"""-m gpu tests of `airlift-align lift`, every GPU step under a time limit of its own (the command through run_lift, the taps and the C ABI in a child
process, tests/helpers/lift_child.py): k_bam_walk / k_lift / k_lift_gather against their host twin and the rules restated in Python through the taps, the
command on the device against `lift --host` at several piece and BGZF block sizes with and without --gpu-deflate, the exact-chain property through the
device, the malformed inputs refused alike by both backends, and no device memory left when a call returns."""
import os
import subprocess
import sys

import pytest

import lift_cases as lc
from select_cases import bgzf
from test_lift_cpu import MALFORMED, check, exact_case, exact_check, run_lift

pytestmark = pytest.mark.gpu


HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "helpers", "lift_child.py")


def run_child(what, d, limit=120):
    """an in-process GPU step (the taps, the C ABI) in a process of its own, under a time limit: a walk that does not advance fails the test"""
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, CHILD, what, str(d)], capture_output=True)
    assert r.returncode == 0, "[%s] exit status %d\n%s\n%s" % (what, r.returncode, r.stdout.decode()[-2000:], r.stderr.decode()[-3000:])
    assert r.stdout.decode().strip().split("\n")[-1].startswith("ok " + what)


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    from airlift_amd import capi
    L = capi.load()
    d = tmp_path_factory.mktemp("gpu_lift")
    chain = str(d / "directed.chain"); open(chain, "w").write(lc.CHAIN)
    return L, d, chain, L.al_dbg_lift_window()             # (a constant of the library: no GPU step)


def test_the_kernels_equal_their_host_twin_and_the_python_rules(env):
    run_child("kernels", env[1])


def test_texts_that_end_inside_a_record(env):
    run_child("ends", env[1])


def test_malformed_input_through_the_taps(env):
    run_child("malformed", env[1])


@pytest.fixture(scope="module")
def cli_case(env):
    L, d, chain, W = env
    recs = lc.directed(257) + lc.walk_sets(W)["long"] + lc.walk_sets(W)["cut1"]
    out = {}
    for block in (700, 0xff00):
        bam = str(d / ("cli%d.bam" % block)); open(bam, "wb").write(bgzf(lc.bam_bytes(lc.HEADER, lc.REFS, recs), block))
        out[block] = bam
    return recs, out


@pytest.mark.parametrize("deflate", [False, True])
@pytest.mark.parametrize("piece", [1000, 4096, None])
@pytest.mark.parametrize("block", [700, 0xff00])
def test_lift_on_the_device_equals_lift_host(env, cli_case, tmp_path, block, piece, deflate):
    L, d, chain, W = env
    recs, bams = cli_case
    extra = (["--piece", str(piece)] if piece else []) + (["--gpu-deflate"] if deflate else [])
    kb = dict(AL_INFLATE_PIECE_KB=2 if piece else 1024, AL_TIMING=1)
    hd = tmp_path / "host"; hd.mkdir()
    rh, out_h, bed_h = run_lift(hd, bams[block], chain, *(["--piece", str(piece)] if piece else []), **kb)
    assert rh.returncode == 0, rh.stderr.decode()[-1500:]
    host_bam, host_bed = lc.decode(out_h), open(bed_h, "rb").read()
    r, out, bed = run_lift(tmp_path, bams[block], chain, *extra, host=False, **kb)
    check(r, out, bed, lc.HEADER, lc.REFS, recs)
    assert lc.decode(out) == host_bam and open(bed, "rb").read() == host_bed
    err = r.stderr.decode()
    assert "(k_lift):" in err and "device bytes held at return: 0\n" in err and "the host twin lifts" not in err, err[-1500:]
    assert "(host twin):" in rh.stderr.decode()
    if deflate:
        assert "BAM output: deflate (device" in err, err[-1500:]


@pytest.mark.parametrize("case", ["worked", "ends", "fold", "letters", "order", "minus", "minus2"])
def test_exact_chain_property_through_the_device(tmp_path, case):
    old, new, refs, recs, bam, chain = exact_case(case, tmp_path)
    r, out, bed = run_lift(tmp_path, bam, chain, "--piece", "4096", host=False, AL_INFLATE_PIECE_KB=2, AL_TIMING=1)
    assert r.returncode == 0 and b"(k_lift):" in r.stderr, r.stderr.decode()[-1500:]
    kept, rows = exact_check(case, out, bed, old, new, refs, recs)
    print(case, "kept", kept, "rows", rows, "of", len(recs))
    if case.startswith("minus"):
        assert kept == 0 and rows == len(recs)
    else:
        assert kept > len(recs) / 2 and rows > len(recs) / 20, (kept, rows, len(recs))


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_input_is_refused_alike_by_both_backends(env, tmp_path, name):
    L, d, chain, W = env
    blob, say = MALFORMED[name]
    bam = str(tmp_path / "bad.bam"); open(bam, "wb").write(bgzf(blob, 700))
    res = []
    for host in (True, False):
        r, out, bed = run_lift(tmp_path, bam, chain, "--piece", "1000", host=host, AL_INFLATE_PIECE_KB=1)
        assert r.returncode == 1 and say in r.stderr.decode() and not os.path.exists(out) and not os.path.exists(bed), r.stderr.decode()[-800:]
        res.append([l for l in r.stderr.decode().split("\n") if l.startswith("ERROR")])
    assert res[0] == res[1] and len(res[0]) == 1


def test_the_c_abi_counts_and_leaves_no_device_memory(env):
    run_child("abi", env[1])

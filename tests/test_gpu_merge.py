"""-m gpu tests of `airlift-align merge`, every GPU step under a time limit of its own (the command through run_merge, the taps and the C ABI in a child
process, tests/helpers/merge_child.py): the keys, the window rule, the merge-path merge and the gather against their host twin and against the rules restated in
Python (merge_cases.py) through the taps, with one round and with the round loop; the command on the device against `--host` and Python over member size, window
size and --gpu-deflate; the refusals on the device path; the C ABI."""
import os
import subprocess
import sys

import pytest

import lift_sort_cases as ls
import merge_cases as mc
from select_cases import bgzf
from test_merge_cpu import check, piece_args, refused, run_merge, write_inputs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "helpers", "merge_child.py")


def run_child(what, d, limit=120):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, CHILD, what, str(d)], capture_output=True)
    assert r.returncode == 0, "[%s] exit status %d\n%s\n%s" % (what, r.returncode, r.stdout.decode()[-2000:], r.stderr.decode()[-3000:])
    assert r.stdout.decode().strip().split("\n")[-1].startswith("ok " + what)


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    from airlift_amd import capi
    L = capi.load()
    return L, tmp_path_factory.mktemp("gpu_merge"), L.al_dbg_merge_tile(), L.al_dbg_lift_window()        # (constants of the library: no GPU step)


def test_the_taps_equal_their_host_twin_and_python(env):
    run_child("taps", env[1])


def test_the_round_loop_equals_its_host_twin_and_python(env):
    run_child("loop", env[1])


def test_the_taps_refuse_what_the_twin_refuses(env):
    run_child("refusals", env[1])


def test_the_c_abi_on_the_device(env):
    run_child("abi", env[1])


@pytest.fixture(scope="module")
def cli_case(env):
    L, d, T, W = env
    return mc.cli_pair(W), {}


@pytest.mark.parametrize("deflate", [False, True])
@pytest.mark.parametrize("piece", [1000, 4096, None])
@pytest.mark.parametrize("block", [700, 0xff00])
def test_merge_on_the_device_equals_host_and_python(env, cli_case, tmp_path, block, piece, deflate):
    L, d, T, W = env
    inputs, host_runs = cli_case
    bams = write_inputs(d, "pair", inputs, block)
    pa, kb = piece_args(piece)
    if (block, piece) not in host_runs:
        rh, out_h = run_merge(d, bams, *pa, AL_TIMING=1, **kb)
        assert rh.returncode == 0 and "(host twin):" in rh.stderr.decode(), rh.stderr.decode()[-1500:]
        host_runs[block, piece] = ls.inflate(out_h)
    r, out = run_merge(tmp_path, bams, *pa, *(["--gpu-deflate"] if deflate else []), host=False, AL_TIMING=1, **kb)
    assert check(r, out, inputs) == host_runs[block, piece]
    err = r.stderr.decode()
    assert "(k_merge):" in err and "device bytes held at return: 0\n" in err and "the host twin merges" not in err, err[-1500:]
    if deflate:
        assert "BAM output: deflate (device" in err, err[-1500:]


@pytest.mark.parametrize("piece", mc.PIECES)
def test_unsorted_input_is_refused_on_the_device(env, tmp_path, piece):
    for name, (inputs, idx) in sorted(mc.unsorted(mc.ENDS["cli700", piece]).items()):
        bams = write_inputs(tmp_path, name, inputs, 700)
        r, out = run_merge(tmp_path, bams, "--piece", str(piece), host=False, AL_INFLATE_PIECE_KB=2)
        refused(r, out, "ERROR: '%s': not in coordinate order at offset %d of the inflated stream" % (bams[1], mc.unsorted_offset(inputs, idx)))


@pytest.mark.parametrize("name", sorted(mc.malformed()))
def test_malformed_input_is_refused_on_the_device(env, tmp_path, name):
    first, blob, say = mc.malformed()[name]
    a = write_inputs(tmp_path, "first", [first], 700)[0]
    b = str(tmp_path / "bad.bam"); open(b, "wb").write(bgzf(blob, 700))
    r, out = run_merge(tmp_path, [a, b], "--piece", "1000", host=False, AL_INFLATE_PIECE_KB=1)
    refused(r, out, "ERROR: '%s': malformed BAM record at " % b + say)


@pytest.mark.parametrize("name", sorted(mc.refs_refusals()) + sorted(mc.header_refusals()))
def test_lists_and_lines_that_do_not_merge_are_refused_on_the_device(env, tmp_path, name):
    inputs, say = dict(mc.refs_refusals(), **mc.header_refusals())[name]
    bams = write_inputs(tmp_path, name, inputs, 700)
    r, out = run_merge(tmp_path, bams, "--piece", "1000", host=False)
    refused(r, out, say)

"""`airlift-align merge --host`: the kernels' host twin behind the command, without a GPU.  Every list of merge_cases.py through the command at BGZF member sizes
700 and 0xff00 and window sizes 1000, 4096 and the default: the inflated output must equal the merged header and the expected records of the Python rules byte
for byte, and bam_util.read_bam must decode it.  The refusals -- unsorted and malformed input, reference lists and @RG lines that do not merge -- give exit
status 1, their message and no output file; the command's argument errors are refused; al_merge_bams through capi with its host flag."""
import os
import subprocess

import pytest

import bam_util
import lift_cases as lc
import lift_sort_cases as ls
import merge_cases as mc
from select_cases import bgzf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
T_GUESS = 1024          # (the CPU tests need no exact tile: the twin has none; the shapes are those of the device tests)
W_GUESS = 8192
LIMIT = 60              # seconds a `merge` process may take
FORMS = [(700, 1000), (0xff00, 4096), (700, None), (0xff00, 1000)]       # (member size, --piece)


def run_merge(d, bams, *extra, host=True, out=None, **env):
    """one `merge` process under a time limit of its own; 124 / 137 as exit status: it hung"""
    out = out or str(d / "merged.bam")
    if os.path.exists(out):
        os.unlink(out)
    e = dict(os.environ); e.update({k: str(v) for k, v in env.items()})
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT), CLI, "merge", "-o", out] + (["--host"] if host else []) + list(extra) + list(bams), capture_output=True, env=e)
    return r, out


def write_inputs(d, tag, inputs, block):
    paths = []
    for i, x in enumerate(inputs):
        p = str(d / ("%s_%d_%d.bam" % (tag, block, i))); paths.append(p)
        if not os.path.exists(p):
            open(p, "wb").write(bgzf(mc.stream(x), block))
    return paths


def piece_args(piece):
    return (["--piece", str(piece)] if piece else []), dict(AL_INFLATE_PIECE_KB=2 if piece else 1024)


def check(r, out, inputs):
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    want = mc.expected_stream(inputs)
    got = ls.inflate(out)
    assert got == want
    text, refs, recs, _ = bam_util.read_bam(out)
    assert text == mc.merged_header(inputs) and refs == mc.merged_refs(inputs)[0] and len(recs) == sum(len(i[2]) for i in inputs)
    return got


def refused(r, out, say):
    err = r.stderr.decode()
    assert r.returncode == 1 and say in err and not os.path.exists(out), err[-1500:]
    assert len([l for l in err.split("\n") if l.startswith("ERROR") or l.startswith("[ERROR]")]) == 1, err[-1500:]


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("merge"), mc.self_check(T_GUESS)


def test_the_case_lists_have_the_properties_they_claim():
    """A self-check of the reference, not of the product: it runs no C++ and passes without the feature; what it guards is that the cases the other tests
    run mean what their comments say, for the tile and the window sizes used."""
    all_ = mc.self_check(T_GUESS)
    assert sorted(all_) == ["headers", "refs", "ties", "tiles", "windows1000", "windows4096"]
    mc.self_check(256); mc.self_check(2048)


@pytest.mark.parametrize("block,piece", FORMS)
@pytest.mark.parametrize("lname", ["tiles", "ties", "refs", "headers", "windows1000", "windows4096"])
def test_every_list_through_the_host_twin(work, lname, block, piece):
    d, all_ = work
    pa, env = piece_args(piece)
    for name, inputs in sorted(all_[lname].items()):
        bams = write_inputs(d, lname + "_" + name, inputs, block)
        r, out = run_merge(d, bams, *pa, AL_TIMING=1, **env)
        check(r, out, inputs)
        err = r.stderr.decode()
        assert "(host twin):" in err and "device bytes held at return: 0\n" in err and " + ".join(str(len(i[2])) for i in inputs) + " records" in err, (name, err[-800:])


def test_small_windows_take_many_rounds_and_refills(work):
    d, all_ = work
    for p in mc.PIECES:
        inputs = all_["windows%d" % p]["dense"]
        r, out = run_merge(d, write_inputs(d, "windows%d_dense" % p, inputs, 700), "--piece", str(p), AL_TIMING=1, AL_INFLATE_PIECE_KB=2)
        check(r, out, inputs)
        err = r.stderr.decode()
        rounds = int(err.split(" rounds")[0].split()[-1]); refills = int(err.split(" refills")[0].split()[-1])
        assert rounds >= 5 and refills >= 6, err[-800:]


def test_the_command_matrix_input(work):
    d, _ = work
    inputs = mc.cli_pair(W_GUESS)
    for block, piece in FORMS:
        pa, env = piece_args(piece)
        r, out = run_merge(d, write_inputs(d, "pair", inputs, block), *pa, "-t", "4", "-l", "1", **env)
        check(r, out, inputs)


@pytest.mark.parametrize("where", ["tap", "cli700"])
@pytest.mark.parametrize("piece", mc.PIECES)
def test_unsorted_input_is_refused(work, tmp_path, piece, where):
    d, _ = work
    for name, (inputs, idx) in sorted(mc.unsorted(mc.ENDS[where, piece]).items()):
        for block in (700, 0xff00):
            bams = write_inputs(tmp_path, name, inputs, block)
            r, out = run_merge(tmp_path, bams, "--piece", str(piece), AL_INFLATE_PIECE_KB=2)
            refused(r, out, "ERROR: '%s': not in coordinate order at offset %d of the inflated stream" % (bams[1], mc.unsorted_offset(inputs, idx)))
    r, out = run_merge(tmp_path, bams[::-1], "--piece", str(piece))                       # the unsorted file as input 1
    refused(r, out, "'%s': not in coordinate order" % bams[1])


@pytest.mark.parametrize("name", sorted(mc.malformed()))
def test_malformed_input_is_refused(tmp_path, name):
    first, blob, say = mc.malformed()[name]
    a = write_inputs(tmp_path, "first", [first], 700)[0]
    b = str(tmp_path / "bad.bam"); open(b, "wb").write(bgzf(blob, 700))
    for pa in (["--piece", "1000"], []):
        r, out = run_merge(tmp_path, [a, b], *pa, AL_INFLATE_PIECE_KB=1)
        refused(r, out, "ERROR: '%s': malformed BAM record at " % b + say)


@pytest.mark.parametrize("name", sorted(mc.refs_refusals()) + sorted(mc.header_refusals()))
def test_lists_and_lines_that_do_not_merge_are_refused(tmp_path, name):
    inputs, say = dict(mc.refs_refusals(), **mc.header_refusals())[name]
    bams = write_inputs(tmp_path, name, inputs, 700)
    r, out = run_merge(tmp_path, bams, "--piece", "1000")
    refused(r, out, say)
    assert bams[1] in r.stderr.decode()


def test_argument_errors(work, tmp_path):
    d, all_ = work
    bams = write_inputs(tmp_path, "arg", all_["ties"]["equal_diff_len"], 700)
    out = str(tmp_path / "o.bam")
    def run(*a):
        return subprocess.run(["timeout", "-k", "10", str(LIMIT), CLI, "merge"] + list(a), capture_output=True)
    r = run("-o", out, "--host", bams[0]); assert r.returncode == 1 and b"2 to 8 input BAMs, not 1" in r.stderr
    r = run("-o", out, "--host", *([bams[0]] * 9)); assert r.returncode == 1 and b"2 to 8 input BAMs, not 9" in r.stderr
    r = run("-o", bams[1], "--host", *bams); assert r.returncode == 1 and b"is also the output" in r.stderr and os.path.getsize(bams[1]) > 28
    r = run("-o", out, "--host", "--gpu-deflate", *bams); assert r.returncode == 1 and b"--host opens no device: it cannot be combined with --gpu-deflate" in r.stderr
    r = run("--host", *bams); assert r.returncode == 1 and b"Usage: airlift-align merge -o OUT.bam" in r.stderr
    r = run("-o", out, "--host", bams[0], str(tmp_path / "missing.bam")); assert r.returncode == 1 and b"failed to open file" in r.stderr
    assert not os.path.exists(out)
    r = subprocess.run([CLI], capture_output=True); assert b"airlift-align merge -o OUT.bam" in r.stderr + r.stdout


def test_the_c_abi_with_the_host_flag(work, tmp_path):
    from airlift_amd import capi
    d, all_ = work
    inputs = all_["windows1000"]["k3"]
    bams = write_inputs(tmp_path, "abi", inputs, 700); out = str(tmp_path / "abi_out.bam")
    st = capi.merge_bams(bams, out, flags=capi.MERGE_HOST, piece_bytes=1000)
    assert ls.inflate(out) == mc.expected_stream(inputs)
    assert st.on_device == 0 and st.held == 0 and st.n_in == 3 and list(st.records_in[:3]) == [len(i[2]) for i in inputs] and st.records == sum(st.records_in[:3]) and st.rounds > 3
    with pytest.raises(capi.AirliftError):
        capi.merge_bams(bams[:1], out, flags=capi.MERGE_HOST)


def test_the_taps_of_the_host_twin(work):
    """al_dbg_merge_host: one round with every input at eof (tags, keys and bytes against Python), and the round loop at both window sizes"""
    from merge_tap import tap
    from airlift_amd import capi
    L = capi.load(); d, all_ = work
    assert L.al_dbg_merge_tile() >= 64
    for lname in ("ties", "refs"):
        for name, inputs in sorted(all_[lname].items()):
            got = tap(L, inputs, 0); e = mc.expected(inputs)
            assert got["rounds"] == 1 and got["tags"] == [i << 28 | x for i, x, _ in e] and got["keys"] == [mc.key(o) for _, _, o in e], name
            assert got["packed"] == b"".join(lc.rec_bytes(o) for _, _, o in e), name
    for p in mc.PIECES:
        for name, inputs in sorted(all_["windows%d" % p].items()):
            got = tap(L, inputs, p); e = mc.expected(inputs)
            assert [t >> 28 for t in got["tags"]] == [i for i, _, _ in e] and got["packed"] == b"".join(lc.rec_bytes(o) for _, _, o in e), (p, name)
            assert got["rounds"] > 1, (p, name)

"""-m gpu tests of --gpu-inflate through the command line: extract-reads and remap read a BAM that the product itself wrote (--sorted-bam, host-deflated
and --gpu-deflate, so that our own compressor's members are read back) through AlBgzfIn and k_inflate; the yardstick is the default reader's output."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")


@pytest.fixture(scope="module")
def case(golden_unpacked, tmp_path_factory):
    d = golden_unpacked["g1_mt150pe"]
    m = json.load(open(os.path.join(d, "meta.json")))
    t = tmp_path_factory.mktemp("gpu_inflate")
    ref = os.path.join(d, m["ref"]); fq = [os.path.join(d, r) for r in m["reads"]]
    bams = {}
    for name, extra in (("host", []), ("dev", ["--gpu-deflate"])):
        bams[name] = str(t / (name + ".bam"))
        r = subprocess.run([CLI, "-ax", "sr", "--sorted-bam"] + extra + ["-o", bams[name], ref] + fq, capture_output=True)
        assert r.returncode == 0, r.stderr.decode()[-1500:]
    sq = [l.split("\t") for l in open(os.path.join(d, "expected.sam")) if l.startswith("@SQ")]
    name, ln = sq[0][1][3:], int(sq[0][2][3:])
    bed = str(t / "regions.bed")
    open(bed, "w").write("".join("%s\t%d\t%d\n" % (name, b, e) for b, e in ((200, 3000), (2500, 6000), (9000, ln - 100))))
    return dict(bams=bams, bed=bed, ref=ref, fq=fq, tmp=t)


def _rows(args, **env):
    return subprocess.run([CLI, "extract-reads"] + args, capture_output=True, env=dict(os.environ, **{k: str(v) for k, v in env.items()}))


@pytest.mark.parametrize("which", ["host", "dev"])
@pytest.mark.parametrize("piece", [None, 4])
def test_extract_reads_equals_the_default_reader(case, which, piece):
    tail = ["--noprune", case["bams"][which], case["bed"]]
    exp = _rows(tail)
    assert exp.returncode == 0 and exp.stdout.count(b"\n") > 500
    got = _rows(["--gpu-inflate"] + tail, AL_TIMING=1, **({"AL_INFLATE_PIECE_KB": piece} if piece else {}))
    assert got.returncode == 0, got.stderr.decode()[-1500:]
    assert got.stdout == exp.stdout
    assert b"BGZF input (k_inflate)" in got.stderr and b" 0 pieces on the host backend" in got.stderr
    pruned = ["--gpu-inflate", case["bams"][which], case["bed"], "150"]
    assert _rows(pruned).stdout == _rows(pruned[1:]).stdout


def test_remap_writes_the_same_sam_files(case):
    t = case["tmp"]; env = dict(os.environ, AL_PG_PLAIN="1")
    out = {}
    for name, extra in (("default", []), ("inflate", ["--gpu-inflate"])):
        p, s = str(t / (name + "_p.sam")), str(t / (name + "_s.sam"))
        r = subprocess.run([CLI, "remap", "--noprune"] + extra + ["-o", p, "--singletons", s, case["ref"], case["bams"]["dev"], case["bed"]] + case["fq"], capture_output=True, env=env)
        assert r.returncode == 0, r.stderr.decode()[-1500:]
        out[name] = (open(p, "rb").read(), open(s, "rb").read())
    assert out["inflate"] == out["default"] and out["default"][0].count(b"\n") > 500


def test_a_refusal_of_device_memory_gives_the_same_rows_and_a_count(case):
    tail = ["--noprune", case["bams"]["dev"], case["bed"]]
    got = _rows(["--gpu-inflate"] + tail, AL_TIMING=1, AL_TEST_INFLATE_NOMEM=1)
    assert got.returncode == 0 and got.stdout == _rows(tail).stdout
    assert got.stderr.count(b"no device memory for the inflater's buffers") == 1
    line = [l for l in got.stderr.decode().split("\n") if "BGZF input" in l][0]
    assert int(line.split(" pieces on the host backend")[0].split()[-1]) > 0


def test_a_corrupt_member_is_an_error_and_no_signal(case):
    data = bytearray(open(case["bams"]["host"], "rb").read())
    data[len(data) // 2] ^= 0x55
    bad = str(case["tmp"] / "corrupt.bam"); open(bad, "wb").write(bytes(data))
    got = _rows(["--gpu-inflate", "--noprune", bad, case["bed"]])
    assert got.returncode == 1, got.returncode
    assert b"BGZF member at file offset" in got.stderr or b"no BGZF member at file offset" in got.stderr or b"truncated BGZF member" in got.stderr

"""-m gpu tests of --gpu-deflate: --bam / --sorted-bam with the BGZF blocks deflated by the device backend of AlBgzf (al_deflate.hip).  The yardstick is the
same command without the switch under the host driver (AL_HOST_IO=1), which tests/test_gpu_bam_stream.py pins: the uncompressed stream and its cut into
blocks must be that file's, and the compressed bytes -- a function of each block's bytes -- the same whatever the batching."""
import json
import os
import re
import subprocess
import zlib

import pytest

from bam_util import read_bam, sam_fields
from deflate_util import BLOCK, EOF_BLOCK, deflate_device, deflate_host, members
from test_gpu_bam_stream import ENVS, _same_record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
SETS = ["g1_mt150pe", "g2_100se", "g3_adversarial"]
MODES = {"bam": ["--bam"], "sorted": ["--sorted-bam"]}
# Size of the --bam file against the same blocks deflated by zlib at level 1 (raw, wbits -15, 26 bytes of member around each): measured on an MI355X
# -- it is a property of the function, the host twin gives the same -- and recorded in DESIGN.md section 5 ("--gpu-deflate: sizes"); the bound is the
# measured ratio with 5 % headroom for a later deliberate retune of the function.
RATIO_VS_ZLIB_1 = {"g1_mt150pe": 1.1653, "g2_100se": 1.0219, "g3_adversarial": 1.0775}


def _run(cmd, cwd, env=None):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return r


def _golden(golden_unpacked, name):
    d = golden_unpacked[name]
    m = json.load(open(os.path.join(d, "meta.json")))
    return d, m, (["-R", m["rg"]] if m.get("rg") else [])


_cache = {}


def _cached(key, cmd, cwd, env):
    if key not in _cache:
        _cache[key] = _run(cmd, cwd, env)
    return _cache[key]


def _cmd(mode, rg, m, extra=()):
    return [CLI, "-ax", "sr", "-t", "8"] + MODES[mode] + list(extra) + rg + [m["ref"]] + m["reads"]


def _host_file(golden_unpacked, name, mode):
    d, m, rg = _golden(golden_unpacked, name)
    return _cached(("host", name, mode), _cmd(mode, rg, m), d, dict(AL_HOST_IO="1", AL_TIMING="1")).stdout


def _plain(golden_unpacked, name, mode):
    d, m, rg = _golden(golden_unpacked, name)
    return _cached(("plain", name, mode), _cmd(mode, rg, m, ["--gpu-deflate"]), d, dict(AL_TIMING="1"))


def _raws(z):
    assert z.endswith(EOF_BLOCK)
    return [r for _, r in members(z)]


@pytest.mark.parametrize("env", list(ENVS), ids=list(ENVS))
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", SETS)
def test_gpu_deflate_keeps_the_stream_and_its_blocks(golden_unpacked, name, mode, env, tmp_path):
    d, m, rg = _golden(golden_unpacked, name)
    host = _raws(_host_file(golden_unpacked, name, mode))
    cmd = _cmd(mode, rg, m, ["--gpu-deflate"])
    r = _run(cmd, d, env=dict(ENVS[env], AL_TIMING="1"))
    assert b"stream pipeline" in r.stderr and b"deflate (device" in r.stderr, r.stderr.decode(errors="replace")[-1500:]
    resident = int(re.search(rb"blocks, (\d+) of them compressed where the batch lay", r.stderr).group(1))
    assert (resident > 0) == (mode == "bam"), "--bam batches are compressed in device memory, the sorted file's bytes come from the host's merge"
    mine = _raws(r.stdout)
    assert [len(x) for x in mine] == [len(x) for x in host]       # the per-member ISIZE lists
    assert mine == host
    assert r.stdout == _plain(golden_unpacked, name, mode).stdout  # the same compressed file under every batching
    out = tmp_path / "o.bam"
    _run(cmd[:5] + ["-o", str(out)] + cmd[5:], d, env=dict(ENVS[env], AL_TIMING="1"))
    assert out.read_bytes() == r.stdout


@pytest.mark.parametrize("name", SETS)
def test_gpu_deflate_bam_decodes_to_the_reference_sam(golden_unpacked, name):
    d, m, rg = _golden(golden_unpacked, name)
    sam = open(os.path.join(d, "expected.sam")).read().split("\n")
    hdr = [l for l in sam if l.startswith("@")]; body = [l for l in sam if l and not l.startswith("@")]
    text, refs, recs, _ = read_bam(_plain(golden_unpacked, name, "bam").stdout)
    assert text == "\n".join(hdr) + "\n"
    names = [n for n, _ in refs]
    assert len(recs) == len(body)
    for b, s in zip(recs, [sam_fields(l, names) for l in body]):
        _same_record(b, s)


@pytest.mark.parametrize("mode", list(MODES))
def test_gpu_deflate_other_drivers_and_paths_give_the_same_file(golden_unpacked, mode, tmp_path):
    """the host driver with the device backend, a batch cut by AL_TEST_NOMEM_ABOVE, a flush the device refuses (the host twin takes it), -l 9, and for the
    sorted file spilled runs: one file"""
    d, m, rg = _golden(golden_unpacked, "g1_mt150pe")
    want = _plain(golden_unpacked, "g1_mt150pe", mode).stdout
    cmd = _cmd(mode, rg, m, ["--gpu-deflate"])
    r = _run(cmd, d, env=dict(AL_HOST_IO="1", AL_TIMING="1"))
    assert b"stream pipeline" not in r.stderr and b"deflate (device" in r.stderr and r.stdout == want
    r = _run(cmd, d, env=dict(AL_TEST_NOMEM_ABOVE="37", AL_TIMING="1"))
    assert b"does not fit the device workspaces" in r.stderr and r.stdout == want
    r = _run(cmd, d, env=dict(AL_TEST_DEFLATE_NOMEM="1", AL_TIMING="1"))
    assert b"this flush is deflated on the host" in r.stderr and r.stdout == want
    assert _run(cmd + ["-l", "9"], d).stdout == want
    if mode == "sorted":
        r = _run(cmd[:6] + ["-K", "30000", "--sort-mem", "100000"] + cmd[6:], d, env=dict(AL_TIMING="1"))
        assert b"spilled runs" in r.stderr and r.stdout == want


@pytest.mark.parametrize("mode", list(MODES))
def test_gpu_deflate_after_the_hand_over_to_the_general_reader(golden_unpacked, mode, tmp_path):
    """a multi-line record mid-file: the host driver continues into the same BGZF stream, device backend included"""
    import airlift_amd as A
    d, m, rg = _golden(golden_unpacked, "g1_mt150pe")
    (n1, s1, q1), (n2, s2, q2) = [A.read_fastx(os.path.join(d, f)) for f in m["reads"]]
    for path, (nm, sq, ql) in ((tmp_path / "a.fq", (n1, s1, q1)), (tmp_path / "b.fq", (n2, s2, q2))):
        with open(path, "wb") as f:
            for i in range(300):
                h = len(sq[i]) // 2
                f.write(b"@" + nm[i] + b"\n" + (sq[i][:h] + b"\n" + sq[i][h:] if i == 140 else sq[i]) + b"\n+\n" + (ql[i][:h] + b"\n" + ql[i][h:] if i == 140 else ql[i]) + b"\n")
    cmd = [CLI, "-ax", "sr", "-t", "4"] + MODES[mode] + rg + [os.path.join(d, m["ref"]), "a.fq", "b.fq"]
    host = _run(cmd, tmp_path, env=dict(AL_HOST_IO="1")).stdout
    r = _run(cmd[:5] + ["--gpu-deflate"] + cmd[5:], tmp_path, env=dict(AL_TIMING="1"))
    assert b"general reader takes over" in r.stderr and b"deflate (device" in r.stderr
    assert _raws(r.stdout) == _raws(host)
    assert r.stdout == _run(cmd[:5] + ["--gpu-deflate"] + cmd[5:], tmp_path, env=dict(AL_HOST_IO="1")).stdout


@pytest.mark.parametrize("mode", list(MODES))
def test_without_the_switch_nothing_changes(golden_unpacked, mode):
    d, m, rg = _golden(golden_unpacked, "g3_adversarial")
    r = _run(_cmd(mode, rg, m), d, env=dict(AL_TIMING="1"))
    assert b"BAM output: deflate (level" in r.stderr and b"deflate (device" not in r.stderr
    assert r.stdout == _host_file(golden_unpacked, "g3_adversarial", mode)


@pytest.mark.parametrize("name", SETS)
def test_gpu_deflate_size(golden_unpacked, name):
    z = _plain(golden_unpacked, name, "bam").stdout
    raws = _raws(z)
    assert len(z) < sum(len(r) + 31 for r in raws) + 28           # smaller than stored
    ref = 28
    for r in raws:
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        ref += 26 + len(c.compress(r) + c.flush())
    ratio = len(z) / ref
    print("size %s: %d bytes in %d blocks -> %d with --gpu-deflate, %d with zlib level 1: ratio %.4f" % (name, sum(map(len, raws)), len(raws), len(z), ref, ratio))
    assert ratio <= RATIO_VS_ZLIB_1[name] * 1.05


@pytest.mark.parametrize("name", ["g1_mt150pe", "g3_adversarial"])
def test_kernel_equals_host_twin_on_a_real_record_stream(golden_unpacked, name):
    data = b"".join(_raws(_host_file(golden_unpacked, name, "bam")))
    assert len(data) > BLOCK
    assert deflate_device(data) == deflate_host(data)

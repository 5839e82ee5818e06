"""-m gpu tests of BGZF-compressed FASTQ through the stream driver (--gpu-inflate on the mapping commands: al_bgzf_take.h, al_stream_append_bgzf,
k_inflate), through the command line.  The BGZF files are made here from the golden sets' plain reads, member by member (inflate_cases.member around
Python zlib's raw deflate).  A case that the stream driver takes shows `stream pipeline` and its `BGZF input` part in the AL_TIMING lines, and its
stdout is byte for byte the run on the plain files, which is the golden SAM."""
import gzip
import json
import os
import re
import subprocess

import pytest

import inflate_cases as ic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
PART = b"stream pipeline: BGZF input ("


def _cli(args, cwd, env=None, ok=True):
    r = subprocess.run([CLI] + args, cwd=cwd, capture_output=True, env=dict(os.environ, **(env or {})))
    if ok:
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return r


def bgzf(data, chunk, eof=True, empty_every=0):
    out = []
    for k, o in enumerate(range(0, len(data), chunk)):
        if empty_every and k and k % empty_every == 0:
            out.append(ic.EOF_BLOCK)                          # (an empty member in the middle)
        c = data[o:o + chunk]
        out.append(ic.member(ic.deflate_raw(c, 6), c))
    return b"".join(out) + (ic.EOF_BLOCK if eof else b"")


@pytest.fixture(scope="module")
def sets(golden_unpacked, tmp_path_factory):
    """per golden set: directory, meta, -R arguments, the reads' plain bytes, the plain run's SAM (asserted equal to the golden once, here), and a work dir"""
    out = {}
    for name in ("g1_mt150pe", "g2_100se"):
        d = golden_unpacked[name]
        m = json.load(open(os.path.join(d, "meta.json")))
        rg = ["-R", m["rg"]] if m.get("rg") else []
        exp = open(os.path.join(d, "expected.sam"), "rb").read()
        ref = os.path.join(d, m["ref"])
        plain = _cli(["-ax", "sr", "-t", "4"] + rg + [ref] + m["reads"], d, env=dict(AL_TIMING="1"))
        assert plain.stdout == exp and b"stream pipeline" in plain.stderr and PART not in plain.stderr
        out[name] = dict(ref=ref, rg=rg, exp=exp, reads=[open(os.path.join(d, f), "rb").read() for f in m["reads"]], tmp=tmp_path_factory.mktemp(name))
    return out


def _write(s, tag, datas):
    names = []
    for i, b in enumerate(datas):
        p = os.path.join(str(s["tmp"]), "%s_%d.fq.gz" % (tag, i + 1))
        if not os.path.exists(p):
            open(p, "wb").write(b)
        names.append(p)
    return names


def _map(s, files, env=None, flag=True, extra=(), ok=True):
    return _cli(["-ax", "sr", "-t", "4"] + (["--gpu-inflate"] if flag else []) + list(extra) + s["rg"] + [s["ref"]] + files, str(s["tmp"]), env=dict(env or {}, AL_TIMING="1"), ok=ok)


def _taken(r):
    assert b"stream pipeline:" in r.stderr and PART + b"k_inflate," in r.stderr, r.stderr[-1500:]
    f = re.search(rb"BGZF input \([^)]*\): (\d+) members in (\d+) launches, (\d+) bytes in, (\d+) bytes out", r.stderr)
    return [int(x) for x in f.groups()]


@pytest.mark.parametrize("piece_kb", ["1", "16"])
@pytest.mark.parametrize("batch", ["64", "301"])
@pytest.mark.parametrize("chunk", [0xff00, 997])
def test_members_batches_and_pieces(sets, chunk, batch, piece_kb):
    """Blocks as bgzip writes them and blocks of 997 bytes (records straddle members, thousands of members), batches whose ends fall inside the inflated
    text, and file pieces smaller than a member / than a few members, so that members straddle pieces."""
    s = sets["g1_mt150pe"]
    files = _write(s, "c%d" % chunk, [bgzf(b, chunk) for b in s["reads"]])
    r = _map(s, files, dict(AL_BATCH_READS=batch, AL_INFLATE_PIECE_KB=piece_kb))
    mem, _, b_in, b_out = _taken(r)
    assert b_in == sum(os.path.getsize(f) for f in files) and b_out == sum(len(b) for b in s["reads"])
    assert mem == sum((len(b) + chunk - 1) // chunk + 1 for b in s["reads"])
    assert r.stdout == s["exp"]


def test_a_single_file(sets):
    s = sets["g2_100se"]
    files = _write(s, "se", [bgzf(s["reads"][0], 0xff00)])
    for env in (dict(), dict(AL_BATCH_READS="64", AL_INFLATE_PIECE_KB="1")):
        r = _map(s, files, env)
        _taken(r)
        assert r.stdout == s["exp"]


def test_one_file_bgzf_and_the_other_plain(sets):
    s = sets["g1_mt150pe"]
    for which in (0, 1):
        datas = [bgzf(b, 0xff00) if i == which else b for i, b in enumerate(s["reads"])]
        files = _write(s, "mixed%d" % which, datas)
        r = _map(s, files, dict(AL_BATCH_READS="301"))
        assert _taken(r)[3] == len(s["reads"][which])
        assert r.stdout == s["exp"]


def test_no_newline_after_the_last_record(sets):
    s = sets["g1_mt150pe"]
    assert all(b.endswith(b"\n") for b in s["reads"])
    cut = [b[:-1] for b in s["reads"]]
    plain = _map(s, _write(s, "noeol_plain", cut), flag=False)
    assert plain.stdout == s["exp"] and PART not in plain.stderr
    for chunk in (0xff00, 997):
        r = _map(s, _write(s, "noeol%d" % chunk, [bgzf(b, chunk) for b in cut]), dict(AL_BATCH_READS="301"))
        assert _taken(r)[3] == sum(len(b) for b in cut)
        assert r.stdout == s["exp"]


def test_empty_members_in_the_middle_and_no_eof_block(sets):
    s = sets["g1_mt150pe"]
    r = _map(s, _write(s, "empties", [bgzf(b, 997, empty_every=3) for b in s["reads"]]), dict(AL_BATCH_READS="301", AL_INFLATE_PIECE_KB="1"))
    _taken(r)
    assert r.stdout == s["exp"]
    r = _map(s, _write(s, "noeof", [bgzf(b, 0xff00, eof=False) for b in s["reads"]]), dict(AL_BATCH_READS="64"))
    _taken(r)
    assert r.stdout == s["exp"]


def test_hand_over_at_an_irregular_record(sets):
    """A multi-line record in the middle: the batch ends in front of it and the general reader continues at that offset of the INFLATED stream (gzseek).
    The output is the host driver's on the same files."""
    s = sets["g1_mt150pe"]
    datas = []
    for b in s["reads"]:
        lines = b.split(b"\n")
        k = 4 * 140                                        # record 140: sequence and quality cut in two lines each
        sq, ql = lines[k + 1], lines[k + 3]
        h = len(sq) // 2
        lines[k:k + 4] = [lines[k], sq[:h], sq[h:], lines[k + 2], ql[:h], ql[h:]]
        datas.append(b"\n".join(lines))
    files = _write(s, "multiline", [bgzf(b, 997) for b in datas])
    host = _map(s, files, dict(AL_HOST_IO="1"))
    assert b"stream pipeline" not in host.stderr
    for env in (dict(AL_BATCH_READS="64"), dict()):
        r = _map(s, files, env)
        _taken(r)
        assert b"general reader takes over" in r.stderr
        assert r.stdout == host.stdout
    assert host.stdout == s["exp"]                         # (a multi-line record is the same record to the kseq grammar)


def test_bam_output(sets, tmp_path):
    s = sets["g1_mt150pe"]
    files = _write(s, "c65280", [bgzf(b, 0xff00) for b in s["reads"]])
    d = os.path.dirname(s["ref"])
    plain = json.load(open(os.path.join(d, "meta.json")))["reads"]
    a, b = str(tmp_path / "plain.bam"), str(tmp_path / "bgzf.bam")
    r0 = _cli(["-ax", "sr", "-t", "4", "--bam", "-l", "3", "-o", a] + s["rg"] + [s["ref"]] + plain, d, env=dict(AL_TIMING="1"))
    assert b"stream pipeline" in r0.stderr and PART not in r0.stderr
    r = _map(s, files, extra=["--bam", "-l", "3", "-o", b])
    _taken(r)
    assert open(a, "rb").read() == open(b, "rb").read() and os.path.getsize(a) > 1000


def test_a_member_with_a_flipped_crc_byte_fails_the_run(sets):
    s = sets["g1_mt150pe"]
    good = bgzf(s["reads"][0], 997)
    sizes = []
    o = 0
    while o < len(good):
        sizes.append(int.from_bytes(good[o + 16:o + 18], "little") + 1); o += sizes[-1]
    at = sum(sizes[:200])                                 # member 200
    bad = bytearray(good); bad[at + sizes[200] - 8] ^= 0x40
    files = _write(s, "crc", [bytes(bad), bgzf(s["reads"][1], 997)])
    r = _map(s, files, dict(AL_BATCH_READS="301"), ok=False)
    assert r.returncode != 0
    assert files[0].encode() in r.stderr and ("file offset %d" % at).encode() in r.stderr and b"CRC mismatch" in r.stderr, r.stderr[-1500:]
    # a cut last member and a chain that breaks: the same
    files = _write(s, "cut", [good[:-40], bgzf(s["reads"][1], 997)])
    r = _map(s, files, ok=False)
    assert r.returncode != 0 and files[0].encode() in r.stderr and re.search(rb"truncated BGZF member at file offset \d+", r.stderr), r.stderr[-1500:]
    files = _write(s, "broken", [good[:at] + b"\x00" + good[at + 1:], bgzf(s["reads"][1], 997)])
    r = _map(s, files, ok=False)
    assert r.returncode != 0 and files[0].encode() in r.stderr and ("no BGZF member at file offset %d" % at).encode() in r.stderr, r.stderr[-1500:]


def test_plain_gzip_files_get_the_notice_and_the_host_driver(sets):
    s = sets["g1_mt150pe"]
    files = _write(s, "gzip", [gzip.compress(b, 6) for b in s["reads"]])
    r = _map(s, files)
    assert r.stderr.count(b"is not a BGZF file; it is read as one gzip stream on the host") == 1
    assert b"stream pipeline" not in r.stderr
    assert r.stdout == s["exp"]


def test_refused_staging_memory_gets_the_notice_and_the_host_driver(sets):
    s = sets["g1_mt150pe"]
    files = _write(s, "c65280", [bgzf(b, 0xff00) for b in s["reads"]])
    r = _map(s, files, dict(AL_TEST_INFLATE_NOMEM="1"))
    assert r.stderr.count(b"--gpu-inflate: no device memory for the inflater's staging buffers") == 1
    assert b"stream pipeline" not in r.stderr
    assert r.stdout == s["exp"]


def test_bgzf_files_without_the_flag_take_the_host_driver(sets):
    """Nothing changes without the flag (this case passes before the feature as well)."""
    s = sets["g1_mt150pe"]
    files = _write(s, "c65280", [bgzf(b, 0xff00) for b in s["reads"]])
    r = _map(s, files, flag=False)
    assert b"stream pipeline" not in r.stderr
    assert r.stdout == s["exp"]

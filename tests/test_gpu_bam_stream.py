"""-m gpu tests of BAM output through the stream driver: the records are made by kernels (k_bam_len / k_bam_write / k_bam_bulk, al_stream.hip, over
al_dev_bam.h) and the host only deflates (--bam) or sorts, merges and deflates (--sorted-bam).  The yardstick is the host driver (AL_HOST_IO=1:
host parser + al_write_bam_rec), itself pinned against the reference's SAM text by test_bam_outputs_match_sam: the files must be the same bytes,
whatever the batching; the decoded records are compared with expected.sam once more directly."""
import gzip
import json
import os
import subprocess
import zlib

import pytest

from bam_directed import directed_reads
from bam_util import read_bam, sam_fields

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
SETS = ["g1_mt150pe", "g2_100se", "g2_250pe", "g3_adversarial", "g6_repeats"]
MODES = {"bam": ["--bam"], "sorted": ["--sorted-bam", "-l", "1"]}
ENVS = {"default": dict(),
        "64_reads_per_batch": dict(AL_BATCH_READS="64", AL_CTXS="1", AL_SLOTS="2", AL_PIECE_MB="1"),
        "301_reads_3_contexts": dict(AL_BATCH_READS="301", AL_CTXS="3", AL_SLOTS="5"),
        "small_out_pieces": dict(AL_OUT_PIECE_MB="1")}


def _run(cmd, cwd, env=None, ok=True):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, env=dict(os.environ, **(env or {})))
    if ok:
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return r


def _golden(golden_unpacked, name):
    d = golden_unpacked[name]
    m = json.load(open(os.path.join(d, "meta.json")))
    return d, m, (["-R", m["rg"]] if m.get("rg") else [])


def _streamed_bam(r):
    assert b"stream pipeline" in r.stderr and b"of BAM records" in r.stderr, "the stream driver did not write the BAM:\n" + r.stderr.decode(errors="replace")[-1500:]
    assert b"BAM output: deflate" in r.stderr


_host_cache = {}


def _host(cmd, cwd, key=None):
    """the same command under the host driver (one run per distinct command and directory)"""
    k = (tuple(cmd), str(cwd)) if key is None else key
    if k not in _host_cache:
        r = _run(cmd, cwd, env=dict(AL_HOST_IO="1", AL_TIMING="1"))
        assert b"stream pipeline" not in r.stderr
        _host_cache[k] = r.stdout
    return _host_cache[k]


@pytest.mark.parametrize("env", list(ENVS), ids=list(ENVS))
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", SETS)
def test_stream_driver_equals_host_driver(golden_unpacked, name, mode, env, tmp_path):
    """To a pipe and to -o FILE, with the default batches, 64 reads per batch on one context and two slots, 301 reads on three contexts, and the
    records leaving the device in 1 MB pieces: batch and piece boundaries must not show in the file."""
    d, m, rg = _golden(golden_unpacked, name)
    cmd = [CLI, "-ax", "sr", "-t", "8"] + MODES[mode] + rg + [m["ref"]] + m["reads"]
    host = _host(cmd, d)
    r = _run(cmd, d, env=dict(ENVS[env], AL_TIMING="1"))
    _streamed_bam(r)
    assert r.stdout == host
    out = tmp_path / "o.bam"
    r = _run(cmd[:5] + ["-o", str(out)] + cmd[5:], d, env=dict(ENVS[env], AL_TIMING="1"))
    _streamed_bam(r)
    assert out.read_bytes() == host


def _same_record(b, s):
    for k in ("qname", "flag", "rid", "pos", "mapq", "cigar", "nrid", "npos", "tlen", "seq", "qual"):
        assert b[k] == s[k], (k, b, s)
    assert len(b["tags"]) == len(s["tags"])
    for x, y in zip(b["tags"], s["tags"]):
        if isinstance(x, tuple):
            assert x[:2] == y[:2] and abs(x[2] - y[2]) < 1e-6, (x, y)
        else:
            assert x == y, (x, y)


@pytest.mark.parametrize("name", SETS)
def test_stream_bam_decodes_to_the_reference_sam(golden_unpacked, name):
    """Not only the host path: header, reference dictionary and every field of every record against expected.sam (printed by the reference build);
    the sorted file holds the mapped records in the stable coordinate order."""
    d, m, rg = _golden(golden_unpacked, name)
    sam = open(os.path.join(d, "expected.sam")).read().split("\n")
    hdr = [l for l in sam if l.startswith("@")]; body = [l for l in sam if l and not l.startswith("@")]
    r = _run([CLI, "-ax", "sr", "-t", "4", "--bam"] + rg + [m["ref"]] + m["reads"], d, env=dict(AL_TIMING="1", AL_BATCH_READS="301"))
    _streamed_bam(r)
    text, refs, recs, n_blocks = read_bam(r.stdout)
    assert text == "\n".join(hdr) + "\n"
    names = [n for n, _ in refs]
    assert [("@SQ\tSN:%s\tLN:%d" % x) for x in refs] == [l for l in hdr if l.startswith("@SQ")]
    assert len(recs) == len(body)
    exp = [sam_fields(l, names) for l in body]
    for b, s in zip(recs, exp):
        _same_record(b, s)
    r = _run([CLI, "-ax", "sr", "-t", "3", "--sorted-bam", "-l", "1"] + rg + [m["ref"]] + m["reads"], d, env=dict(AL_TIMING="1", AL_BATCH_READS="301"))
    _streamed_bam(r)
    text2, refs2, recs2, _ = read_bam(r.stdout)
    assert text2 == "@HD\tVN:1.6\tSO:coordinate\n" + text and refs2 == refs
    keep = [s for s in exp if not (s["flag"] & 4)]
    keys = [(b["rid"], b["pos"]) for b in recs2]
    assert keys == sorted(keys) and len(recs2) == len(keep)
    order = sorted(range(len(keep)), key=lambda i: (keep[i]["rid"], keep[i]["pos"]))     # stable, like the device radix sort
    for b, i in zip(recs2, order):
        _same_record(b, keep[i])


@pytest.mark.parametrize("opts", [["-Y"], ["--MD"], ["--cs"], ["--secondary=yes"], ["--sam-hit-only"], ["-R", "@RG\\tID:other\\tSM:x"], ["-Y", "--cs", "--secondary=yes"]],
                         ids=["Y", "MD", "cs", "secondary", "hit_only", "R", "Y_cs_secondary"])
def test_stream_bam_output_options(golden_unpacked, opts):
    d, m, rg = _golden(golden_unpacked, "g3_adversarial")
    if "-R" in opts:
        rg = []
    for mode in MODES:
        cmd = [CLI, "-ax", "sr", "-t", "4"] + MODES[mode] + opts + rg + [m["ref"]] + m["reads"]
        r = _run(cmd, d, env=dict(AL_TIMING="1", AL_BATCH_READS="500"))
        _streamed_bam(r)
        assert r.stdout == _host(cmd, d), (mode, opts)


def _write_fq(path, recs):
    with open(path, "wb") as f:
        for n, s, q in recs:
            f.write(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n")


@pytest.fixture(scope="module")
def directed(golden_unpacked, tmp_path_factory):
    d, m, _ = _golden(golden_unpacked, "g1_mt150pe")
    ref = os.path.join(d, m["ref"])
    seq = b"".join(l.strip() for l in open(ref, "rb").read().split(b"\n")[1:])
    pe1, pe2, se = directed_reads(seq)
    t = tmp_path_factory.mktemp("directed")
    _write_fq(t / "a.fq", pe1); _write_fq(t / "b.fq", pe2); _write_fq(t / "se.fq", se)
    _write_fq(t / "il.fq", [x for p in zip(pe1, pe2) for x in p])
    return dict(dir=t, ref=ref, pe1=pe1, pe2=pe2, se=se)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", ["two_files", "interleaved", "single_end"])
def test_stream_bam_directed_reads(directed, shape, mode):
    """Reads made for the corners of the record (tests/bam_directed.py): one- and two-base unmapped reads, odd and even lengths, IUPAC / lowercase /
    U / bytes >= 128 on both strands, hard-clipped supplementary records of odd and even length, /1 /2 names, a 254-byte name -- as two files, as
    one interleaved file and single-end."""
    t = directed["dir"]
    reads = {"two_files": ["a.fq", "b.fq"], "interleaved": ["il.fq"], "single_end": ["se.fq"]}[shape]
    cmd = [CLI, "-ax", "sr", "-t", "4"] + MODES[mode] + ["-R", "@RG\\tID:d\\tSM:d", directed["ref"]] + reads
    host = _host(cmd, t)
    for env in (dict(), dict(AL_BATCH_READS="7", AL_CTXS="2")):
        r = _run(cmd, t, env=dict(env, AL_TIMING="1"))
        _streamed_bam(r)
        assert r.stdout == host, env
    if mode == "bam":   # the reads are what they were made to be
        _, _, recs, _ = read_bam(host)
        sup = [b for b in recs if b["flag"] & 0x800]
        assert {len(b["seq"]) % 2 for b in sup if "H" in b["cigar"]} == {0, 1}, "hard-clipped supplementary records of odd and of even length"
        assert {len(b["seq"]) for b in recs if b["flag"] & 4 and b["seq"] != "*"} >= {1, 2}
        assert any(len(b["qname"]) == 254 for b in recs)
        assert any(b["flag"] & 0x10 and set(b["seq"]) - set("ACGTN") for b in recs) and any(not b["flag"] & 0x14 and set(b["seq"]) - set("ACGTN") for b in recs)
        if shape != "single_end":
            assert all(not b["qname"].endswith(("/1", "/2")) for b in recs)


def _inflate_what_is_there(raw):
    out = b""; p = 0
    while p + 18 <= len(raw):
        bsize = int.from_bytes(raw[p + 16:p + 18], "little") + 1
        if p + bsize > len(raw):
            break
        out += zlib.decompress(raw[p + 18:p + bsize - 8], -15); p += bsize
    return out


@pytest.mark.parametrize("mode", list(MODES))
def test_stream_bam_refuses_a_255_byte_name(directed, mode, tmp_path):
    """l_read_name holds 254 bytes and the NUL: the length pass counts such reads, the driver prints the host writer's message, exits non-zero and
    writes nothing of that batch."""
    pe1, pe2 = list(directed["pe1"]), list(directed["pe2"])
    bad = b"Q" * 255
    pe1[12] = (bad + b"/1",) + pe1[12][1:]; pe2[12] = (bad + b"/2",) + pe2[12][1:]
    _write_fq(tmp_path / "a.fq", pe1); _write_fq(tmp_path / "b.fq", pe2)
    cmd = [CLI, "-ax", "sr", "-t", "4"] + MODES[mode] + [directed["ref"], "a.fq", "b.fq"]
    msg = b"read name longer than 254 characters cannot be stored in BAM: " + b"Q" * 40 + b"..."
    host = _run(cmd, tmp_path, env=dict(AL_HOST_IO="1"), ok=False)
    assert host.returncode != 0 and msg in host.stderr
    for env in (dict(), dict(AL_BATCH_READS="10")):      # the pair is in the only batch / in the third batch
        r = _run(cmd, tmp_path, env=dict(env, AL_TIMING="1"), ok=False)
        assert r.returncode != 0 and msg in r.stderr, r.stderr.decode(errors="replace")[-1500:]
        got = _inflate_what_is_there(r.stdout)
        assert bad[:200] not in got
        for n, _, _ in pe1[10:]:                          # no record of the batch the name is in (10 reads per batch: pairs 10 .. 14), nor of a later one
            assert n[:-2] + b"\0" not in got


@pytest.mark.parametrize("mode", list(MODES))
def test_stream_bam_hands_over_to_the_general_reader(golden_unpacked, mode, tmp_path):
    """The irregular text of test_stream_equals_host_driver_on_irregular_text: CRLF line ends and a comment after the name are strict four-line
    FASTQ; a multi-line record mid-file is not -- the host driver continues at that byte into the same BGZF stream / sort store."""
    import airlift_amd as A
    d, m, rg = _golden(golden_unpacked, "g1_mt150pe")
    (n1, s1, q1), (n2, s2, q2) = [A.read_fastx(os.path.join(d, f)) for f in m["reads"]]
    ref = os.path.join(d, m["ref"])

    def write(path, names, seqs, quals, style):
        with open(path, "wb") as f:
            for i in range(len(names)):
                nm, s, q = names[i], seqs[i], quals[i]
                if style == "multiline" and i == 140:
                    h = len(s) // 2
                    f.write(b"@" + nm + b"\n" + s[:h] + b"\n" + s[h:] + b"\n+\n" + q[:h] + b"\n" + q[h:] + b"\n")
                else:
                    f.write(b"@" + nm + b" a comment\r\n" + s + b"\r\n+" + nm + b"\r\n" + q + b"\r\n")

    for style, resume in (("crlf", False), ("multiline", True)):
        write(tmp_path / "a.fq", n1[:300], s1[:300], q1[:300], style)
        write(tmp_path / "b.fq", n2[:300], s2[:300], q2[:300], style)
        cmd = [CLI, "-ax", "sr", "-t", "4"] + MODES[mode] + rg + [ref, "a.fq", "b.fq"]
        host = _host(cmd, tmp_path, key=(mode, style))
        for extra in (dict(), dict(AL_BATCH_READS="50")):
            r = _run(cmd, tmp_path, env=dict(extra, AL_TIMING="1"))
            _streamed_bam(r)
            assert (b"general reader takes over" in r.stderr) == resume, (style, r.stderr[-600:])
            assert r.stdout == host, (style, extra)
        assert len(read_bam(host)[2]) >= (600 if mode == "bam" else 300)


@pytest.mark.parametrize("mode", list(MODES))
def test_stream_bam_cuts_a_batch_that_does_not_fit(golden_unpacked, mode):
    """AL_ERR_NOMEM in the stream driver (test_stream_cuts_a_batch_that_does_not_fit): the pieces of the batch are kept on the host and go into the
    BGZF stream / the store in order."""
    d, m, rg = _golden(golden_unpacked, "g1_mt150pe")
    cmd = [CLI, "-ax", "sr"] + MODES[mode] + rg + [m["ref"]] + m["reads"]
    r = _run(cmd, d, env=dict(AL_TEST_NOMEM_ABOVE="37", AL_TIMING="1"))
    _streamed_bam(r)
    assert b"does not fit the device workspaces" in r.stderr
    assert r.stdout == _host(cmd, d)


def test_stream_sorted_bam_spilled_runs(golden_unpacked):
    """--sort-mem far below the output: sorted runs are spilled while batches arrive and merged at the end; the file is the unspilled run's."""
    d, m, rg = _golden(golden_unpacked, "g1_mt150pe")
    cmd = [CLI, "-ax", "sr", "-t", "4", "--sorted-bam", "-K", "30000"] + rg + [m["ref"]] + m["reads"]
    whole = _run(cmd, d, env=dict(AL_TIMING="1"))
    _streamed_bam(whole)
    assert b"merging" not in whole.stderr
    r = _run(cmd[:6] + ["--sort-mem", "100000"] + cmd[6:], d, env=dict(AL_TIMING="1"))
    _streamed_bam(r)
    assert b"spilled runs" in r.stderr
    assert r.stdout == whole.stdout
    assert len(gzip.decompress(whole.stdout)) > 500000

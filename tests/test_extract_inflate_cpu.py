"""extract-reads --gpu-inflate with the reader's host backend (AL_TEST_INFLATE_HOST=1: AlBgzfIn lists the members of every piece and zlib inflates them
on worker threads; no device): the rows are those of the default reader, whatever the piece size, and a damaged file is error -2 with a message."""
import gzip
import os
import random
import struct
import subprocess
import zlib

import pytest

import inflate_cases as ic
from test_extract_cpu import write_bam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")


def bgzf(blob, block, eof=True):
    return b"".join(ic.member(ic.deflate_raw(blob[o:o + block], 6), blob[o:o + block]) for o in range(0, len(blob), block)) + (ic.EOF_BLOCK if eof else b"")


def run(args, **env):
    e = dict(os.environ, AL_TEST_INFLATE_HOST="1"); e.update({k: str(v) for k, v in env.items()})
    return subprocess.run([CLI, "extract-reads"] + args, capture_output=True, env=e)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("inflate_n1")
    rng = random.Random(11)
    refs = [("chr1", 200000), ("chr2", 100000)]
    recs = []
    for i in range(3000):
        rid = rng.randrange(2); pos = rng.randrange(0, refs[rid][1] - 3000)
        if i % 150 == 7:       # a record longer than three small members: a name of 250 characters and a CIGAR of 600 operations
            recs.append((rid, pos, rng.choice([0, 60]), 1 | 64, [(1, "M"), (1, "I")] * 300, "long" + "x" * 242 + "%04d" % i, 900))
        else:
            cig = [(150, "M")] if rng.random() < 0.6 else [(70, "M"), (2, "D"), (80, "M")]
            recs.append((rid, pos, rng.choice([0, 5, 11, 60]), 1 | (64 if i & 1 else 128), cig, "read%d" % (i // 2), 150))
    recs.sort(key=lambda r: (r[0], r[1]))
    plain = str(d / "plain.bam"); write_bam(plain, refs, recs)
    blob = gzip.decompress(open(plain, "rb").read())
    paths = {"plain": plain}
    for name, data in (("big", bgzf(blob, 0xff00)), ("small", bgzf(blob, 700)), ("noeof", bgzf(blob, 20000, eof=False))):
        paths[name] = str(d / (name + ".bam")); open(paths[name], "wb").write(data)
    whole = bgzf(blob, 20000)
    paths["truncated"] = str(d / "truncated.bam"); open(paths["truncated"], "wb").write(whole[:len(whole) - 28 - 100])
    k = len(ic.member(ic.deflate_raw(blob[:20000], 6), blob[:20000]))          # the second member's CRC32 field
    k2 = k + len(ic.member(ic.deflate_raw(blob[20000:40000], 6), blob[20000:40000]))
    paths["crc"] = str(d / "crc.bam"); open(paths["crc"], "wb").write(whole[:k2 - 8] + bytes([whole[k2 - 8] ^ 1]) + whole[k2 - 7:])
    paths["crc_offset"] = k
    bed = str(d / "regions.bed")
    with open(bed, "w") as f:
        for _ in range(40):
            c = rng.randrange(2); b = rng.randrange(0, refs[c][1] - 9000); f.write("%s\t%d\t%d\n" % (refs[c][0], b, b + rng.randrange(500, 9000)))
    paths["bed"] = bed
    return paths


@pytest.mark.parametrize("prune", [True, False])
@pytest.mark.parametrize("which,piece", [("big", None), ("big", 16), ("small", 1), ("small", 3), ("noeof", None)])
def test_rows_equal_the_default_readers(case, prune, which, piece):
    tail = ([] if prune else ["--noprune"]) + [case[which], case["bed"], "150"]
    exp = run(tail)
    assert exp.returncode == 0 and exp.stdout.count(b"\n") > 50
    assert b"long" in exp.stdout or prune
    got = run(["--gpu-inflate", "-t", "4"] + tail, **({"AL_INFLATE_PIECE_KB": piece} if piece else {}))
    assert got.returncode == 0, got.stderr.decode()
    assert got.stdout == exp.stdout


def test_the_timing_line_counts_members_and_bytes(case):
    got = run(["--gpu-inflate", case["small"], case["bed"], "150"], AL_TIMING=1, AL_INFLATE_PIECE_KB=2)
    assert got.returncode == 0
    line = [l for l in got.stderr.decode().split("\n") if "BGZF input" in l]
    assert len(line) == 1 and " members in " in line[0] and "%d bytes in" % os.path.getsize(case["small"]) in line[0]


def test_a_truncated_file_is_an_error_with_a_message(case):
    got = run(["--gpu-inflate", case["truncated"], case["bed"], "150"])
    assert got.returncode == 1 and b"truncated BGZF member at file offset" in got.stderr


def test_a_wrong_crc_is_an_error_that_names_the_member(case):
    got = run(["--gpu-inflate", case["crc"], case["bed"], "150"])
    assert got.returncode == 1
    assert ("BGZF member at file offset %d: status 10" % case["crc_offset"]).encode() in got.stderr


def test_a_plain_gzip_bam_takes_the_stream_reader_with_a_notice(case):
    tail = [case["plain"], case["bed"], "150"]
    exp = run(tail); got = run(["--gpu-inflate"] + tail)
    assert got.returncode == 0 and got.stdout == exp.stdout and exp.stdout
    assert b"is not a BGZF file" in got.stderr and b"is not a BGZF file" not in exp.stderr


def test_the_library_entry_returns_minus_two(case, tmp_path):
    import ctypes as C
    code = ("import ctypes as C, sys\nfrom airlift_amd import capi\nL = capi.load()\nlibc = C.CDLL(None); libc.fopen.restype = C.c_void_p; libc.fopen.argtypes = [C.c_char_p, C.c_char_p]\n"
            "f = libc.fopen(sys.argv[3].encode(), b'wb')\nprint(L.al_extract_reads_ex(sys.argv[1].encode(), sys.argv[2].encode(), 150, 1, f, 1, -1, 2))\n")
    import sys
    r = subprocess.run([sys.executable, "-c", code, case["crc"], case["bed"], str(tmp_path / "rows")], capture_output=True, cwd=ROOT, env=dict(os.environ, AL_TEST_INFLATE_HOST="1"))
    assert r.returncode == 0 and r.stdout.strip() == b"-2", r.stderr.decode()

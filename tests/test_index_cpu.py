"""`airlift-align bam-index --host`: the kernels' host twin behind the command, without a GPU.  Every case of index_cases.py -- at BGZF member sizes 700 and
0xff00, with members cut at record boundaries and with an empty member in the middle -- through the command at piece sizes 1000, 4096 and the default: the file
written must equal the index of the Python rules byte for byte, and the query procedure of the SAM specification over the written file must find exactly the
records a scan finds.  The host tap; the C ABI with its host flag; the refusals, each with its message and no output file; merge --write-index and
lift --sorted --write-index against bam-index of their outputs."""
import os
import subprocess

import pytest

import index_cases as ic
import lift_cases as lc
import merge_cases as mc
from select_cases import bgzf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
LIMIT = 60              # seconds a process may take
PIECE_FORMS = [1000, 4096, None]


def piece_args(piece):
    return (["--piece", str(piece)] if piece else []), dict(AL_INFLATE_PIECE_KB=2 if piece else 1024)


def run_index(bam, *extra, host=True, out=None, **env):
    """one `bam-index` process under a time limit of its own; 124 / 137 as exit status: it hung"""
    target = out or bam + ".bai"
    if os.path.exists(target):
        os.unlink(target)
    e = dict(os.environ); e.update({k: str(v) for k, v in env.items()})
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT), CLI, "bam-index"] + (["--host"] if host else []) + list(extra) + [bam] + ([out] if out else []), capture_output=True, env=e)
    return r, target


def write_case(d, name, recs, layout):
    p = str(d / (name.replace("@", "_") + ".bam"))
    data = ic.compress(ic.stream(recs), layout)
    if not os.path.exists(p):
        open(p, "wb").write(data)
    return p, data


def refused(r, target, say):
    err = r.stderr.decode()
    assert r.returncode == 1 and say in err and not os.path.exists(target), err[-1500:]
    assert len([l for l in err.split("\n") if l.startswith("ERROR") or l.startswith("[ERROR]")]) == 1, err[-1500:]
    assert not [f for f in os.listdir(os.path.dirname(target)) if ".tmp." in f]


def cli_end(piece):
    """where the first text of the command ends for 700-byte members: whole members from the one that holds the first record until the piece is covered"""
    return 700 * (ic.H0 // 700 + -(-piece // 700))


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("index"), ic.self_check()


def test_the_case_lists_have_the_shapes_they_claim_and_answer_queries():
    """A self-check of the reference, not of the product: it runs no C++ and passes without the feature; it guards that the cases mean what their comments say and
    that the index the rules define answers every region of the fixed list as a scan does."""
    assert len(ic.self_check()) >= 28


@pytest.mark.parametrize("piece", PIECE_FORMS)
def test_every_case_through_the_host_twin(work, piece):
    d, cases = work
    pa, env = piece_args(piece)
    for name, (recs, layout) in sorted(cases.items()):
        bam, data = write_case(d, name, recs, layout)
        r, target = run_index(bam, *pa, AL_TIMING=1, **env)
        assert r.returncode == 0, (name, r.stderr.decode()[-1500:])
        got = open(target, "rb").read()
        assert got == ic.expected_bai(ic.REFS, recs, ic.members(data)), (name, piece)
        err = r.stderr.decode()
        assert "(host twin):" in err and "device bytes held at return: 0\n" in err and " %d records" % len(recs) in err, (name, err[-800:])
        for k in ("file read", "copy up", "inflate", "walk", "keys", "assemble"):
            assert k + " " in err, (k, err[-800:])


def test_small_pieces_take_many_pieces_and_one_bin_stays_one_chunk(work):
    d, cases = work
    recs, layout = cases["one_bin@700"]
    bam, data = write_case(d, "one_bin@700", recs, layout)
    for piece, least in ((1000, 10), (4096, 3)):
        r, target = run_index(bam, "--piece", str(piece), AL_TIMING=1, AL_INFLATE_PIECE_KB=2)
        assert r.returncode == 0, r.stderr.decode()[-1500:]
        err = r.stderr.decode()
        assert int(err.split(" pieces")[0].split()[-1]) >= least, err[-800:]
        contigs, _ = ic.parse_bai(open(target, "rb").read())
        assert [len(c) for c in contigs[0]["bins"].values()] == [1]                       # the run crossed every piece boundary and is one chunk


def test_queries_over_the_written_files_find_what_a_scan_finds(work):
    d, cases = work
    for name in ("boundaries@700", "basics@700", "basics@65280", "bin_return_two_members", "empty_member", "spans_three_members"):
        recs, layout = cases[name]
        bam, data = write_case(d, name, recs, layout)
        r, target = run_index(bam, "--piece", "1000", AL_INFLATE_PIECE_KB=2)
        assert r.returncode == 0, r.stderr.decode()[-1500:]
        bai = open(target, "rb").read()
        for rid, beg, end in ic.regions():
            assert ic.query(bai, data, rid, beg, end) == ic.scan(recs, rid, beg, end), (name, rid, beg, end)


def test_the_output_name_and_the_no_op_index(work, tmp_path):
    d, cases = work
    recs, layout = cases["basics@700"]
    bam, data = write_case(tmp_path, "named", recs, layout)
    r, target = run_index(bam, out=str(tmp_path / "other.bai"))
    assert r.returncode == 0 and open(target, "rb").read() == ic.expected_bai(ic.REFS, recs, ic.members(data)) and not os.path.exists(bam + ".bai")
    assert sorted(os.listdir(str(tmp_path))) == ["named.bam", "other.bai"]                # (the temporary name is gone)
    r = subprocess.run([CLI, "index", bam], capture_output=True)
    assert r.returncode == 0 and not os.path.exists(bam + ".bai")                          # `bwa index REF` stays the accepted no-op
    r = subprocess.run([CLI, "bam-index", "--host"], capture_output=True); assert r.returncode == 1 and b"Usage: airlift-align bam-index" in r.stderr
    r = subprocess.run([CLI, "bam-index", "--host", str(tmp_path / "missing.bam")], capture_output=True); assert r.returncode == 1 and b"failed to open file" in r.stderr
    r = subprocess.run([CLI, "bam-index", "--host", bam, bam], capture_output=True); assert r.returncode == 1 and b"is also the output" in r.stderr and os.path.getsize(bam) == len(data)
    r = subprocess.run([CLI], capture_output=True); assert b"airlift-align bam-index" in r.stderr + r.stdout


def test_the_taps_of_the_host_twin(work):
    from airlift_amd import capi
    L = capi.load(); d, cases = work
    for name, (recs, layout) in sorted(cases.items()):
        blob = ic.stream(recs); data = ic.compress(blob, layout); mem = ic.members(data)
        want = ic.expected_bai(ic.REFS, recs, mem)
        for piece in (0, 1000, 4096, 97):
            assert ic.tap(L, blob, mem, len(data), piece) == want, (name, piece)


def test_the_c_abi_with_the_host_flag(work, tmp_path):
    from airlift_amd import capi
    d, cases = work
    recs, layout = cases["basics@700"]
    bam, data = write_case(tmp_path, "abi", recs, layout)
    st = capi.index_bam(bam, flags=capi.BAI_HOST, piece_bytes=200)
    want = ic.expected_bai(ic.REFS, recs, ic.members(data))
    assert open(bam + ".bai", "rb").read() == want
    assert st.on_device == 0 and st.held == 0 and st.records == len(recs) and st.unplaced == 3 and st.pieces > 1 and st.bai_bytes == len(want) and st.chunks >= 5
    with pytest.raises(capi.AirliftError):
        capi.index_bam(str(tmp_path / "missing.bam"), flags=capi.BAI_HOST)


@pytest.mark.parametrize("name", sorted(ic.refusals()))
def test_input_without_an_index_is_refused(tmp_path, name):
    recs, say = ic.refusals()[name]
    for block in ic.BLOCKS:
        bam = str(tmp_path / ("%s_%d.bam" % (name, block))); open(bam, "wb").write(bgzf(ic.stream(recs), block))
        for pa in (["--piece", "1000"], []):
            r, target = run_index(bam, *pa, AL_INFLATE_PIECE_KB=2)
            refused(r, target, "ERROR: '%s': " % bam + say)
    if name == "beyond_2_29":
        assert "the BAI format ends there, and a CSI index is not built" in r.stderr.decode()


@pytest.mark.parametrize("piece", ic.PIECES)
def test_a_descent_across_a_piece_boundary_is_refused(tmp_path, piece):
    recs, off = ic.boundary_descent(cli_end(piece))
    assert mc.first_window(ic.stream(recs), ic.H0, cli_end(piece))[1] == off              # the record that descends is the first of the second text
    bam = str(tmp_path / "boundary.bam"); open(bam, "wb").write(bgzf(ic.stream(recs), 700))
    r, target = run_index(bam, "--piece", str(piece), AL_INFLATE_PIECE_KB=2)
    refused(r, target, "ERROR: '%s': not in coordinate order at offset %d of the inflated stream" % (bam, off))


@pytest.mark.parametrize("name", sorted(mc.malformed()))
def test_malformed_input_is_refused(tmp_path, name):
    _, blob, say = mc.malformed()[name]
    bam = str(tmp_path / "bad.bam"); open(bam, "wb").write(bgzf(blob, 700))
    for pa in (["--piece", "1000"], []):
        r, target = run_index(bam, *pa, AL_INFLATE_PIECE_KB=1)
        refused(r, target, "ERROR: '%s': malformed BAM record at " % bam + say)


def test_a_record_whose_cigar_does_not_fit_is_refused(tmp_path):
    recs = sorted(lc.directed(40), key=mc.key)                                             # (lift's list is not in order: the same shape among records that are)
    h = lc.header_bytes(lc.HEADER, lc.REFS); b = bytearray(lc.rec_bytes(recs[7])); off7 = len(h) + sum(len(lc.rec_bytes(r)) for r in recs[:7])
    import struct
    struct.pack_into("<H", b, 16, 60000)
    blob = h + b"".join(lc.rec_bytes(r) for r in recs[:7]) + bytes(b) + b"".join(lc.rec_bytes(r) for r in recs[8:])
    bam = str(tmp_path / "fit.bam"); open(bam, "wb").write(bgzf(blob, 700))
    r, target = run_index(bam, "--piece", "1000")
    refused(r, target, "ERROR: '%s': malformed BAM record at offset %d of the inflated stream: the name and the CIGAR do not fit" % (bam, off7))


def test_a_file_that_is_not_bgzf_is_refused(tmp_path):
    import gzip
    p = str(tmp_path / "plain.bam"); open(p, "wb").write(gzip.compress(ic.stream(ic.basics())))       # gzip, but no BGZF members
    r, target = run_index(p)
    refused(r, target, "is not a BGZF file")
    q = str(tmp_path / "text.bam"); open(q, "wb").write(b"@HD\tVN:1.6\n" * 20)
    r, target = run_index(q)
    refused(r, target, "is not a BGZF file")


def run_cmd(args, **env):
    e = dict(os.environ); e.update({k: str(v) for k, v in env.items()})
    return subprocess.run(["timeout", "-k", "10", str(LIMIT), CLI] + args, capture_output=True, env=e)


def test_merge_write_index(work, tmp_path):
    inputs = mc.windows(1000)["k3"]
    bams = []
    for i, x in enumerate(inputs):
        bams.append(str(tmp_path / ("in%d.bam" % i))); open(bams[-1], "wb").write(bgzf(mc.stream(x), 700))
    plain, with_ix = str(tmp_path / "plain.bam"), str(tmp_path / "ix.bam")
    r = run_cmd(["merge", "--host", "-o", plain, "--piece", "1000"] + bams, AL_INFLATE_PIECE_KB=2); assert r.returncode == 0 and not os.path.exists(plain + ".bai"), r.stderr.decode()[-1500:]
    r = run_cmd(["merge", "--host", "--write-index", "-o", with_ix, "--piece", "1000"] + bams, AL_INFLATE_PIECE_KB=2, AL_TIMING=1); assert r.returncode == 0, r.stderr.decode()[-1500:]
    assert open(plain, "rb").read() == open(with_ix, "rb").read()                           # the flag changes no byte of the BAM
    assert "[airlift] bam-index: '%s' into '%s.bai' (host twin):" % (with_ix, with_ix) in r.stderr.decode()
    r2, target = run_index(plain)
    assert r2.returncode == 0 and open(target, "rb").read() == open(with_ix + ".bai", "rb").read()
    contigs, no_coor = ic.parse_bai(open(target, "rb").read())
    assert contigs[0]["pseudo"][2] == sum(len(i[2]) for i in inputs) and no_coor == 0


def test_lift_sorted_write_index(tmp_path):
    import lift_sort_cases as ls
    recs = lc.directed(257)
    bam = str(tmp_path / "in.bam"); open(bam, "wb").write(bgzf(lc.bam_bytes(lc.HEADER, lc.REFS, recs), 700))
    chain = str(tmp_path / "c.chain"); open(chain, "w").write(lc.CHAIN)
    plain, with_ix = str(tmp_path / "plain.bam"), str(tmp_path / "ix.bam")
    base = ["lift", "--host", "--chain", chain, "--sorted", "--piece", "4096"]
    r = run_cmd(base + ["-o", plain, "--unmapped-bed", str(tmp_path / "a.bed"), bam]); assert r.returncode == 0 and not os.path.exists(plain + ".bai"), r.stderr.decode()[-1500:]
    r = run_cmd(base + ["--write-index", "-o", with_ix, "--unmapped-bed", str(tmp_path / "b.bed"), bam]); assert r.returncode == 0, r.stderr.decode()[-1500:]
    assert open(plain, "rb").read() == open(with_ix, "rb").read() and open(str(tmp_path / "a.bed"), "rb").read() == open(str(tmp_path / "b.bed"), "rb").read()
    r2, target = run_index(plain)
    assert r2.returncode == 0 and open(target, "rb").read() == open(with_ix + ".bai", "rb").read()
    contigs, no_coor = ic.parse_bai(open(target, "rb").read())
    n = len(ls.split_records(ls.inflate(plain)))
    assert no_coor + sum(c["pseudo"][2] + c["pseudo"][3] for c in contigs if c["pseudo"]) == n and n > 100
    r = run_cmd(["lift", "--host", "--chain", chain, "--write-index", "-o", str(tmp_path / "no.bam"), "--unmapped-bed", str(tmp_path / "no.bed"), bam])
    assert r.returncode == 1 and b"--write-index goes with --sorted" in r.stderr and not os.path.exists(str(tmp_path / "no.bam"))

"""PAF output without a GPU: al_write_paf (the host restatement of mm_write_paf3, format.c:304-330) on hand-made records against lines
the fork printed (tests/golden/g9_paf), the device formatter (al_dev_paf.h) compiled for the CPU against al_write_paf on random
records, the flag values, and the command line: the new options are parsed, the combinations PAF cannot serve exit 1 with a message
before any device is opened."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")


@pytest.fixture(scope="module")
def lib():
    import airlift_amd as A
    L = A.load()
    # contig names and lengths of the g3 / g6 sets' references as far as the lines below need them (the bases do not matter to PAF)
    names = [b"chr1", b"chr2", b"chr3"]
    seqs = [b"ACGT" * 25000] * 3
    idx = L.al_idx_str(10, 15, 3, (C.c_char_p * 3)(*seqs), (C.c_char_p * 3)(*names))
    assert idx
    yield A, L, idx
    L.al_idx_destroy(idx)


def _reg(A, cig=None, **kw):
    r = A.Reg()
    for k, v in kw.items():
        setattr(r, k, v)
    keep = None
    if cig:
        import re
        ops = [(int(n) << 4) | "MIDNSHP=XB".index(o) for n, o in re.findall(r"(\d+)([MIDNSHP=XB])", cig)]
        keep = (C.c_uint32 * len(ops))(*ops)
        r.n_cigar = len(ops); r.cigar = C.cast(keep, C.POINTER(C.c_uint32))
    return r, keep


def test_flag_values():
    import airlift_amd as A
    assert (A.AL_F_OUT_CG, A.AL_F_PAF_NO_HIT, A.AL_F_NO_PRINT_2ND, A.AL_F_CIGAR) == (0x20, 0x8000000, 0x4000, 0x4)     # the fork's MM_F_* (minimap.h:8-38)
    assert A.AL_F_OUT_PAF == 1 << 32                                                                                  # ours: above the fork's bits
    hdr = open(os.path.join(ROOT, "include", "airlift.h")).read()
    for n, v in [("AL_F_OUT_CG", "0x020"), ("AL_F_PAF_NO_HIT", "0x8000000"), ("AL_F_OUT_PAF", "0x100000000LL")]:
        assert "#define %-18s %s" % (n, v) in hdr


# lines of tests/golden/g9_paf (g3_adversarial: paf, c_sec, c, cs, nohit), with the record that must print them
HAND = [
    ("map_only_primary", b"realigned_0/2", dict(qs=0, qe=147, rev=1, rid=2, rs=23722, re=23869, mlen=117, blen=147, mapq=60, id=0, parent=0, cnt=14, score=160, subsc=86), None, 0, None,
     b"realigned_0/2\t150\t0\t147\t-\tchr3\t100000\t23722\t23869\t117\t147\t60\ttp:A:P\tcm:i:14\ts1:i:160\ts2:i:86\trl:i:0\n"),
    ("aligned_secondary_cg", b"realigned_0/1", dict(qs=0, qe=104, rev=0, rid=0, rs=4542, re=4648, mlen=99, blen=106, mapq=0, id=1, parent=0, cnt=4, score=86, dp_max=142, dp_score=142, n_ambi=0),
     "71M2D33M", "CG", None,
     b"realigned_0/1\t150\t0\t104\t+\tchr1\t100000\t4542\t4648\t99\t106\t0\tNM:i:7\tms:i:142\tAS:i:142\tnn:i:0\ttp:A:S\tcm:i:4\ts1:i:86\tde:f:0.0571\trl:i:0\tcg:Z:71M2D33M\n"),
    ("aligned_primary_ambiguous_base", b"realigned_0/2", dict(qs=0, qe=150, rev=1, rid=2, rs=23719, re=23869, mlen=148, blen=149, mapq=60, id=0, parent=0, cnt=14, score=160, subsc=86, dp_max=287, dp_score=289, n_ambi=1),
     "150M", "CG", None,
     b"realigned_0/2\t150\t0\t150\t-\tchr3\t100000\t23719\t23869\t148\t149\t60\tNM:i:2\tms:i:287\tAS:i:289\tnn:i:1\ttp:A:P\tcm:i:14\ts1:i:160\ts2:i:86\tde:f:0.0067\trl:i:0\tcg:Z:150M\n"),
    ("cs_without_cg", b"realigned_0/2", dict(qs=0, qe=150, rev=1, rid=2, rs=23719, re=23869, mlen=148, blen=149, mapq=60, id=0, parent=0, cnt=14, score=160, subsc=86, dp_max=287, dp_score=289, n_ambi=1),
     "150M", "CS", b":108*ca:16*gn:24",
     b"realigned_0/2\t150\t0\t150\t-\tchr3\t100000\t23719\t23869\t148\t149\t60\tNM:i:2\tms:i:287\tAS:i:289\tnn:i:1\ttp:A:P\tcm:i:14\ts1:i:160\ts2:i:86\tde:f:0.0067\trl:i:0\tcs:Z::108*ca:16*gn:24\n"),
]


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_write_paf_hand_records_print_the_forks_lines(lib, case):
    A, L, idx = lib
    _, qname, fields, cig, opt, tag, want = case
    r, keep = _reg(A, cig, **fields)
    flag = {0: 0, "CG": A.AL_F_OUT_CG, "CS": A.AL_F_OUT_CS}[opt]
    assert A.write_paf(idx, qname, 150, r, flag, 0, tag) == want
    if cig:   # the same record with no option set prints neither cg:Z nor the tag; MD wins over cs (format.c:327-328)
        assert b"cg:Z" not in A.write_paf(idx, qname, 150, r, 0, 0, None)
        assert A.write_paf(idx, qname, 150, r, A.AL_F_OUT_CS | A.AL_F_OUT_MD, 0, b"150").endswith(b"\tMD:Z:150\n")
    else:     # no CIGAR (map-only): cg / cs / MD requests print nothing (format.c:321, 327 need r->p)
        assert A.write_paf(idx, qname, 150, r, A.AL_F_OUT_CG | A.AL_F_OUT_MD, 0, b"150") == want


def test_write_paf_no_hit_line_and_rep_len(lib):
    A, L, idx = lib
    assert A.write_paf(idx, b"realigned_23/1", 150, None, 0, 0) == b"realigned_23/1\t150\t0\t0\t*\t*\t0\t0\t0\t0\t0\t0\trl:i:0\n"     # g3_adversarial__nohit
    assert A.write_paf(idx, b"r", 7, None, 0, -1) == b"r\t7\t0\t0\t*\t*\t0\t0\t0\t0\t0\t0\n"                                           # mm_write_paf (rep_len < 0)
    r, _ = _reg(A, None, qs=1, qe=5, rid=1, rs=10, re=14, mlen=4, blen=4, mapq=3, id=2, parent=0, cnt=1, score=4, split=2)
    assert A.write_paf(idx, b"r", 7, r, 0, -1) == b"r\t7\t1\t5\t+\tchr2\t100000\t10\t14\t4\t4\t3\ttp:A:S\tcm:i:1\ts1:i:4\tzd:i:2\n"
    buf = C.create_string_buffer(8)
    assert L.al_write_paf(buf, 8, idx, b"a_long_read_name", 7, None, 0, -1, None) == -1                                              # too small a buffer is an error, not a cut line


@pytest.mark.parametrize("seed", [5, 23, 2026])
def test_device_paf_formatter_equals_al_write_paf(seed):
    """al_dbg_paf_selftest: the formatter k_paf_len / k_paf_write run, compiled for the CPU, against al_write_paf on random reads (hits
    with and without CIGAR, flipped mates, secondaries, no hits, every option): same bytes, and the count pass predicts them."""
    import airlift_amd as A
    assert A.load().al_dbg_paf_selftest(seed, 8000) == 0


def test_cli_takes_the_paf_options():
    """Parsed, not 'ignored', in the main argv loop and in remap's."""
    for opt in ["--paf", "-c", "--paf-no-hit", "--secondary=yes", "--secondary=no"]:
        r = subprocess.run([CLI, "-x", "sr", opt, "/nonexistent/missing.fa"], capture_output=True)
        assert b"ignored" not in r.stderr, (opt, r.stderr)
    r = subprocess.run([CLI, "remap", "--paf", "-c", "--secondary=yes", "--paf-no-hit", "-o", "/nonexistent/o.paf", "a", "b", "c", "d"], capture_output=True)
    assert b"Usage: airlift-align remap" in r.stderr and b"ignored" not in r.stderr
    r = subprocess.run([CLI, "-x", "sr", "--secondary=maybe", "/nonexistent/missing.fa"], capture_output=True)
    assert b"only accepts 'yes' or 'no'" in r.stderr


REJECTED = [["mem", "--paf"], ["samse", "--paf"], ["aln", "--paf"], ["tokens", "--paf", "--read-size", "100", "--skip", "50"],
            ["-ax", "sr", "--paf", "--bam"], ["-ax", "sr", "--sorted-bam", "--paf", "-c"], ["-ax", "sr", "--paf", "--count-candidates"]]


@pytest.mark.parametrize("args", REJECTED, ids=[" ".join(a) for a in REJECTED])
def test_cli_rejects_paf_where_it_cannot_be_written(args, tmp_path):
    """Exit status 1 and a message; decided before the reference is read or a device opened: the paths do not exist and no HIP device
    is visible, and the only complaint is about the combination."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([CLI] + args + [str(tmp_path / "ref.fa"), str(tmp_path / "a.fq"), str(tmp_path / "b.fq")], capture_output=True, env=env, timeout=60)
    assert r.returncode == 1 and r.stdout == b""
    assert b"--paf" in r.stderr and b"cannot be combined with" in r.stderr
    assert b"failed to open" not in r.stderr and b"HIP" not in r.stderr and b"hip" not in r.stderr

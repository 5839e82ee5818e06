"""--MD / --cs / --eqx / -Y output options without a GPU: the C-ABI flag values, al_gen_MD / al_gen_cs (mm_gen_MD / mm_gen_cs) on hand-built
records against hand-written strings, the Python restatement (tests/tags_util.py) against the same strings, and the two SAM formatters
(device routine compiled for the CPU, host al_write_sam_ex) agreeing on -Y and on the spliced tag."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tags_util import md_cs, eqx, nt4, cigar_ops  # noqa: E402

# contig "ctg": 40 bases; the cases below align reads to [10, 30)
REF = "ACGTACGTAC" + "GGATCCNNAT" + "TAGCTAGGCA" + "TTTTACGTAC"
COMP = str.maketrans("ACGTNacgtn", "TGCANtgcan")


def rc(s):
    return s.translate(COMP)[::-1]


def _ops(cig):
    return [(n, "MIDNSHP=X".index(o)) for n, o in cigar_ops(cig)]


# (name, read in sequencing orientation, qs, qe, rs, re, rev, CIGAR, MD, cs short, cs long); the aligned query of a reverse-strand
# record is the reverse complement of read[qs:qe]
CASES = [
    ("forward_exact", "GGATCCNNAT", 0, 10, 10, 20, 0, "10M", "10", ":10", "=GGATCCNNAT"),
    ("n_vs_n_and_n_vs_base", "GNATCCNAAT", 0, 10, 10, 20, 0, "10M", "1G5N2", ":1*gn:5*na:2", "=G*gn=ATCCN*na=AT"),
    ("first_base_mismatch", "TGATCCNNAT", 0, 10, 10, 20, 0, "10M", "0G9", "*gt:9", "*gt=GATCCNNAT"),
    ("deletion_after_mismatch", "GGATCANAT", 0, 9, 10, 20, 0, "6M1D3M", "5C0^N3", ":5*ca-n:3", "=GGATC*ca-n=NAT"),
    ("insertion_and_clip", "xxGGATTCCNNAT", 2, 13, 10, 20, 0, "4M1I6M", "10", ":4+t:6", "=GGAT+t=CCNNAT"),
    ("reverse_strand", rc("GGATCCNNTT"), 0, 10, 10, 20, 1, "10M", "8A1", ":8*at:1", "=GGATCCNN*at=T"),
    ("eqx_ops", "GGATCCNNTT", 0, 10, 10, 20, 0, "6=2=1X1=", "8A1", ":6:2*at:1", "=GGATCC=NN*at=T"),
]


@pytest.fixture(scope="module")
def lib():
    import airlift_amd as A
    L = A.load()
    names = (C.c_char_p * 1)(b"ctg"); seqs = (C.c_char_p * 1)(REF.encode())
    idx = L.al_idx_str(10, 15, 1, seqs, names)
    assert idx
    yield A, L, idx
    L.al_idx_destroy(idx)


def test_flag_values():
    import airlift_amd as A
    assert (A.AL_F_OUT_CS, A.AL_F_OUT_CS_LONG, A.AL_F_SOFTCLIP, A.AL_F_OUT_MD, A.AL_F_EQX) == (0x40, 0x800, 0x80000, 0x1000000, 0x4000000)
    hdr = open(os.path.join(ROOT, "include", "airlift.h")).read()
    for n, v in [("AL_F_OUT_CS", "0x40"), ("AL_F_OUT_CS_LONG", "0x800"), ("AL_F_SOFTCLIP", "0x80000"), ("AL_F_OUT_MD", "0x1000000"), ("AL_F_EQX", "0x4000000")]:
        assert "#define %-18s %s\n" % (n, v) in hdr


def _reg(A, qs, qe, rs, re_, rev, cig):
    ops = _ops(cig)
    arr = (C.c_uint32 * len(ops))(*[n << 4 | o for n, o in ops])
    r = A.Reg(); r.rid = 0; r.qs = qs; r.qe = qe; r.rs = rs; r.re = re_; r.rev = rev; r.n_cigar = len(ops)
    r.cigar = C.cast(arr, type(r.cigar))
    return r, arr


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gen_md_cs_hand_cases(lib, case):
    A, L, idx = lib
    name, read, qs, qe, rs, re_, rev, cig, md, cs_s, cs_l = case
    r, keep = _reg(A, qs, qe, rs, re_, rev, cig)
    assert A.gen_tag(idx, r, read.encode(), "MD") == md.encode()
    assert A.gen_tag(idx, r, read.encode(), "cs", True) == cs_s.encode()
    assert A.gen_tag(idx, r, read.encode(), "cs", False) == cs_l.encode()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_hand_cases(case):
    name, read, qs, qe, rs, re_, rev, cig, md, cs_s, cs_l = case
    q = read[qs:qe]
    if rev:
        q = rc(q)
    t, qq, ops = nt4(REF[rs:re_]), nt4(q), cigar_ops(cig)
    assert md_cs(t, qq, ops, "MD") == md
    assert md_cs(t, qq, ops, "cs") == cs_s
    assert md_cs(t, qq, ops, "cs", long_cs=True) == cs_l


def test_restatement_eqx():
    t, q = nt4("GGATCCNNAT"), nt4("GGTTCCNNTT")
    assert eqx(t, q, [(10, "M")]) == [(2, "="), (1, "X"), (5, "="), (1, "X"), (1, "=")]
    assert eqx(t, nt4("GGATTCCNNAT"), [(4, "M"), (1, "I"), (6, "M")]) == [(4, "="), (1, "I"), (6, "=")]


def test_gen_md_growth_of_the_callers_buffer(lib):
    A, L, idx = lib
    r, keep = _reg(A, 0, 10, 10, 20, 0, "10M")
    buf = C.c_char_p(None); ml = C.c_int(0)
    n = L.al_gen_cs(None, C.byref(buf), C.byref(ml), idx, C.byref(r), b"GGATCCNNAT", 0)
    assert n == 11 and ml.value >= 12 and C.string_at(buf, n) == b"=GGATCCNNAT"
    n2 = L.al_gen_MD(None, C.byref(buf), C.byref(ml), idx, C.byref(r), b"GGATCCNNAT")   # reuses (realloc) the same buffer
    assert n2 == 2 and C.string_at(buf, n2) == b"10"
    libc = C.CDLL(None); libc.free.argtypes = [C.c_void_p]; libc.free(C.cast(buf, C.c_void_p))


@pytest.mark.parametrize("seed", [3, 17, 2026])
def test_formatters_agree_on_softclip_and_tags(seed):
    """al_dbg_sam_selftest draws -Y and MD / cs (with made-up tag values) for a share of its fragments: the device formatter compiled
    for the CPU and al_write_sam_ex must print the same bytes, and the count pass must predict them."""
    import airlift_amd as A
    L = A.load()
    L.al_dbg_sam_selftest.argtypes = [C.c_uint64, C.c_int]; L.al_dbg_sam_selftest.restype = C.c_int
    assert L.al_dbg_sam_selftest(seed, 6000) == 0


def test_cli_accepts_the_output_options_without_warning(tmp_path):
    """The four options are parsed (not 'ignored'), in the main argv loop and in remap's."""
    import subprocess
    cli = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
    for opt in ["--MD", "--cs", "--cs=long", "--cs=none", "-Y", "--eqx"]:
        r = subprocess.run([cli, "-ax", "sr", opt, str(tmp_path / "missing.fa")], capture_output=True)
        assert b"ignored" not in r.stderr, (opt, r.stderr)
    r = subprocess.run([cli, "remap", "--MD", "--eqx", "-Y", "--cs=long", "-o", str(tmp_path / "o.sam"), "a", "b", "c", "d"], capture_output=True)
    assert b"Usage: airlift-align remap" in r.stderr and b"ignored" not in r.stderr         # four positionals: the options were taken, not counted
    r = subprocess.run([cli, "-ax", "sr", "--cs=bogus", str(tmp_path / "missing.fa")], capture_output=True)
    assert b"--cs only takes 'short' or 'long'" in r.stderr

"""CPU tests of `airlift-align lift --host` (the host twin of al_dev_lift.h behind the driver of al_lift.h) against the rules restated in Python
(lift_cases.py): record by record and row by row over the directed sets and tests/golden/g13_lift, at several piece and BGZF block sizes; the header; every
refusal; and, on the exact chain files of tests/golden/g12_exact, the property that the bases under a lifted read are the same in both references."""
import json
import os
import subprocess

import pytest

import lift_cases as lc
from select_cases import bgzf
from test_extract_cpu import write_bam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
G13 = os.path.join(ROOT, "tests", "golden", "g13_lift")
G12 = os.path.join(ROOT, "tests", "golden", "g12_exact")
W_GUESS = 8192          # (the CPU tests need no exact window: the twin has none; the shapes are those of the device tests)


LIMIT = 60              # seconds a `lift` process may take (the largest input here is 100 KB)


def run_lift(d, bam, chain, *extra, host=True, **env):
    """one `lift` process under a time limit of its own; 124 / 137 as exit status: it hung"""
    out, bed = str(d / "out.bam"), str(d / "out.bed")
    for f in (out, bed):
        if os.path.exists(f):
            os.unlink(f)
    e = dict(os.environ); e.update({k: str(v) for k, v in env.items()})
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT), CLI, "lift", "--chain", chain, "-o", out, "--unmapped-bed", bed] + (["--host"] if host else []) + list(extra) + [bam], capture_output=True, env=e)
    return r, out, bed


def check(r, out, bed, header, refs, recs, chain_text=lc.CHAIN):
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    v, kept, rows = lc.lift_all(chain_text, refs, recs)
    text, new_refs, got = lc.decode(out)
    tab = lc.Table(chain_text)
    assert new_refs == list(zip(tab.q_names, tab.q_sizes))
    assert text == lc.lift_header(header, tab)
    assert len(got) == len(kept)
    for g, k in zip(got, kept):
        assert g == lc.as_read_bam(k)
    assert open(bed).read() == "".join(x + "\n" for x in rows)
    return v


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("lift")
    chain = str(d / "directed.chain"); open(chain, "w").write(lc.CHAIN)
    return d, chain


@pytest.mark.parametrize("n", lc.SIZES)
def test_directed_sets_equal_the_python_rules(work, n):
    d, chain = work
    recs = lc.directed(n)
    bam = str(d / ("d%d.bam" % n)); open(bam, "wb").write(bgzf(lc.bam_bytes(lc.HEADER, lc.REFS, recs), 0xff00))
    r, out, bed = run_lift(d, bam, chain)
    v = check(r, out, bed, lc.HEADER, lc.REFS, recs)
    if n >= 63:
        assert v.count(lc.KEPT) > 10 and v.count(lc.UNLIFTED) > 10 and v.count(lc.UNMAPPED) >= 4


def test_the_pool_meets_every_rule():
    """A self-check of the reference, not of the product: the directed records do what their comments in lift_cases.py say under the Python rules alone.  It
    runs no C++ and no kernel, so it passes without the feature; what it guards is that the restatement the other tests compare against means what it says."""
    recs = lc.directed(len(lc.POOL)); v, kept, rows = lc.lift_all(lc.CHAIN, lc.REFS, recs)
    by = {}
    for r, a in zip(recs, v):
        by.setdefault(r["qname"].split("_")[0], []).append(a)
    assert v[:9] == [0, 0, 0, 1, 1, 1, 0, 0, 1] and v[9:14] == [1, 1, 1, 1, 1] and v[14:19] == [0, 1, 0, 0, 1]
    k = {(x["qname"].split("_")[0], x["flag"] & 192): x for x in kept}
    assert (k["pairA", 64]["pos"], k["pairA", 64]["npos"], k["pairA", 64]["tlen"]) == (700, 900, 300)
    assert (k["pairB", 64]["tlen"], k["pairB", 128]["tlen"], k["pairB", 128]["pos"]) == (1000, -1000, 1600)
    assert (k["pairC", 64]["nrid"], k["pairC", 64]["npos"], k["pairC", 64]["tlen"], k["pairC", 64]["flag"]) == (-1, -1, 0, 1 | 8 | 64) and by["pairC"] == [0, 1]
    assert (k["pairD", 64]["nrid"], k["pairD", 64]["npos"], k["pairD", 128]["rid"], k["pairD", 128]["pos"]) == (1, 1500, 1, 1500)
    assert (k["pairE", 128]["rid"], k["pairE", 128]["pos"], k["pairE", 128]["bin"]) == (0, 700, lc.reg2bin(700, 701)) and k["pairE", 64]["npos"] == 500
    assert (k["pairF", 64]["rid"], k["pairF", 64]["pos"], k["pairF", 64]["bin"], k["pairF", 64]["flag"]) == (-1, -1, 4680, 4 | 1 | 64 | 8)
    assert k["pairH", 64]["flag"] == 1 | 8 | 64 and k["pairI", 64]["tlen"] == 0
    assert "chrA\t1120\t1220\tpairC_0.2\t30\t100M" in rows and "chrB\t1500\t1600" in "".join(rows) and "chrA\t600\t601" not in "".join(rows) and "chrA\t1150\t1151\t" in "".join(rows)


@pytest.mark.parametrize("piece", [1000, 4096, None])
@pytest.mark.parametrize("block", [700, 0xff00])
def test_piece_and_block_sizes(work, piece, block):
    d, chain = work
    recs = lc.directed(257) + lc.walk_sets(W_GUESS)["long"]
    bam = str(d / ("p%d.bam" % block)); open(bam, "wb").write(bgzf(lc.bam_bytes(lc.HEADER, lc.REFS, recs), block))
    r, out, bed = run_lift(d, bam, chain, *(["--piece", str(piece)] if piece else []), AL_INFLATE_PIECE_KB=2 if piece else 1024)
    check(r, out, bed, lc.HEADER, lc.REFS, recs)


@pytest.mark.parametrize("name", ["cut0", "cut1", "cut2", "cut3", "long"])
def test_walk_shapes_and_pieces_that_end_inside_a_size_field(work, name):
    d, chain = work
    recs = lc.walk_sets(W_GUESS)[name]
    blob = lc.bam_bytes(lc.HEADER, lc.REFS, recs)
    offs, o = [], len(lc.header_bytes(lc.HEADER, lc.REFS))
    for r in recs:
        offs.append(o); o += len(lc.rec_bytes(r))
    cuts = [offs[k] + (k % 4) for k in range(1, len(offs))]                # members that end 0, 1, 2 and 3 bytes into a block_size field
    bam = str(d / ("w_%s.bam" % name)); open(bam, "wb").write(lc.bgzf_at(blob, cuts))
    r, out, bed = run_lift(d, bam, chain, "--piece", "1", AL_INFLATE_PIECE_KB=1)     # a piece is one member; a long record is a piece with no complete record
    check(r, out, bed, lc.HEADER, lc.REFS, recs)


@pytest.mark.parametrize("name", sorted(lc.HEADERS))
def test_header_rewriting(work, name):
    d, chain = work
    recs = lc.directed(5)
    bam = str(d / ("h_%s.bam" % name)); open(bam, "wb").write(bgzf(lc.bam_bytes(lc.HEADERS[name], lc.REFS, recs), 90))      # (the header spans members)
    r, out, bed = run_lift(d, bam, chain)
    check(r, out, bed, lc.HEADERS[name], lc.REFS, recs)
    text = lc.decode(out)[0]
    assert text.count("@SQ") == 3 and "SO:coordinate" not in text and "SO:queryname" not in text
    if name == "full":
        assert text == "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:newA\tLN:12000\n@SQ\tSN:newB\tLN:3000\n@SQ\tSN:newC\tLN:700\n@PG\tID:x\tPN:x\n"


def test_golden_g13(work, tmp_path):
    exp = json.load(open(os.path.join(G13, "expected.json")))
    for case, e in sorted(exp.items()):
        r, out, bed = run_lift(tmp_path, os.path.join(G13, e["bam"]), os.path.join(G13, e["chain"]), "--piece", "4096", AL_INFLATE_PIECE_KB=2)
        assert r.returncode == 0, r.stderr.decode()[-1500:]
        text, refs, got = lc.decode(out)
        assert text == e["header"] and [list(x) for x in refs] == e["refs"] and open(bed).read() == e["bed"]
        assert [[g[k] for k in e["fields"]] for g in got] == e["records"]
        assert len(got) > 20 and e["bed"].count("\n") > 5
    # ... and the rules of lift_cases.py still say what the fixture holds
    recs = lc.directed(257); e = exp["directed257"]
    assert lc.decode(os.path.join(G13, e["bam"]))[2] == [lc.as_read_bam(r) for r in recs] and open(os.path.join(G13, e["chain"])).read() == lc.CHAIN
    v, kept, rows = lc.lift_all(lc.CHAIN, lc.REFS, recs)
    assert v == e["verdicts"] and "".join(x + "\n" for x in rows) == e["bed"] and [[lc.as_read_bam(k)[f] for f in e["fields"]] for k in kept] == e["records"]


def test_the_twin_takes_over_with_one_notice_when_the_device_or_its_memory_is_refused(work, tmp_path):
    d, chain = work
    recs = lc.directed(257)
    bam = str(tmp_path / "in.bam"); open(bam, "wb").write(bgzf(lc.bam_bytes(lc.HEADER, lc.REFS, recs), 700))
    r, out, bed = run_lift(tmp_path, bam, chain, "--piece", "4096", host=False, AL_TEST_INFLATE_NOMEM=1, AL_TIMING=1, AL_INFLATE_PIECE_KB=2)
    check(r, out, bed, lc.HEADER, lc.REFS, recs)
    err = r.stderr.decode()
    assert err.count("the host twin lifts the reads") == 1 and "(host twin):" in err and "device bytes held at return: 0\n" in err, err[-1500:]


# ---- refusals: exit 1, a message, no output files -------------------------------------------------------------------------------------------------------------
def refused(r, out, bed, *say):
    assert r.returncode == 1, (r.returncode, r.stderr.decode()[-800:])
    for s in say:
        assert s in r.stderr.decode(), r.stderr.decode()[-800:]
    assert not os.path.exists(out) and not os.path.exists(bed)


CHAIN_REFUSALS = {
    "two_qsizes": (lc.CHAIN.replace("newA 12000 - 6000", "newA 12001 - 6000"), ":9: qName 'newA' has qSize 12001 here and 12000 at line 1"),
    "tstrand": (lc.CHAIN.replace("chrB 8000 + 4000", "chrB 8000 - 4000"), ":12: tStrand is not '+'"),
    "size0": (lc.CHAIN.replace("\n900 50 0\n", "\n0 50 0\n"), ":3: size is 0"),
    "beyond_tsize": (lc.CHAIN.replace("\n2850\n", "\n9000\n"), ":4: the block ends beyond tSize"),
    "beyond_qsize": (lc.CHAIN.replace("newC 700 + 100 600", "newC 700 + 300 800"), ":15: a block of this chain ends beyond qSize"),
    "qstrand": (lc.CHAIN.replace("newC 700 + 100", "newC 700 * 100"), ":15: qStrand is neither '+' nor '-'"),
    "data_first": ("100\n" + lc.CHAIN, ":1: an alignment line before the first chain header"),
    "fields": (lc.CHAIN.replace("\n900 50 0\n", "\n900 50\n"), ":3: an alignment line has 1 or 3 fields"),
}


@pytest.mark.parametrize("name", sorted(CHAIN_REFUSALS))
def test_chain_files_that_are_refused(work, tmp_path, name):
    d, _ = work
    text, say = CHAIN_REFUSALS[name]
    chain = str(tmp_path / "bad.chain"); open(chain, "w").write(text)
    bam = str(tmp_path / "in.bam"); open(bam, "wb").write(bgzf(lc.bam_bytes(lc.HEADER, lc.REFS, lc.directed(10)), 0xff00))
    r, out, bed = run_lift(tmp_path, bam, chain)
    refused(r, out, bed, "bad.chain" + say)


def test_wrong_reference_missing_files_and_other_gzip(work, tmp_path):
    d, chain = work
    recs = lc.directed(10)
    bam = str(tmp_path / "wrong.bam"); open(bam, "wb").write(bgzf(lc.bam_bytes(lc.HEADER, [("chrA", 10001)] + lc.REFS[1:], recs), 0xff00))
    refused(*run_lift(tmp_path, bam, chain), "contig 'chrA' has length 10001 in the BAM and tSize 10000 in the chain file: wrong reference")
    gz = str(tmp_path / "gz.bam"); write_bam(gz, lc.REFS, [(0, 500, 30, 0, [(100, "M")], "a", 0)])
    refused(*run_lift(tmp_path, gz, chain), "is not a BGZF file")
    refused(*run_lift(tmp_path, str(tmp_path / "none.bam"), chain), "failed to open file")
    refused(*run_lift(tmp_path, bam, str(tmp_path / "none.chain")), "none.chain: cannot be opened")
    sam = str(tmp_path / "text.bam"); open(sam, "wb").write(bgzf(b"@HD\tVN:1.6\nr\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n", 0xff00))
    refused(*run_lift(tmp_path, sam, chain), "not a BAM file")
    cut = str(tmp_path / "cut.bam"); open(cut, "wb").write(bgzf(lc.bam_bytes(lc.HEADER, lc.REFS, [])[:60], 0xff00))
    refused(*run_lift(tmp_path, cut, chain), "the file ends inside the BAM header")
    r = subprocess.run([CLI, "lift", "--chain", chain, bam], capture_output=True, timeout=LIMIT)
    assert r.returncode == 1 and b"Usage: airlift-align lift --chain CHAIN -o OUT.bam --unmapped-bed FILE" in r.stderr
    r = subprocess.run([CLI, "extract-reads", "--chain", chain, bam, bam], capture_output=True, timeout=LIMIT)
    assert r.returncode == 1 and b"--chain names the chain file of a tokens run" in r.stderr


MALFORMED = lc.malformed()


@pytest.mark.parametrize("piece", [None, 1000])
@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_records_are_refused_with_their_offset(work, tmp_path, name, piece):
    d, chain = work
    blob, say = MALFORMED[name]
    bam = str(tmp_path / "bad.bam"); open(bam, "wb").write(bgzf(blob, 700))
    r, out, bed = run_lift(tmp_path, bam, chain, *(["--piece", str(piece)] if piece else []), AL_INFLATE_PIECE_KB=1)
    refused(r, out, bed, say)


def test_broken_bgzf_members_are_refused(work, tmp_path):
    d, chain = work
    z = bytearray(bgzf(lc.bam_bytes(lc.HEADER, lc.REFS, lc.directed(200)), 700))
    z[2500] ^= 0x55
    bam = str(tmp_path / "crc.bam"); open(bam, "wb").write(bytes(z))
    r, out, bed = run_lift(tmp_path, bam, chain)
    refused(r, out, bed, "BGZF member at file offset")
    bam2 = str(tmp_path / "trunc.bam"); open(bam2, "wb").write(bgzf(lc.bam_bytes(lc.HEADER, lc.REFS, lc.directed(200)), 700)[:-40])
    refused(*run_lift(tmp_path, bam2, chain), "truncated BGZF member at file offset")


# ---- the property on exact chain files: the bases under a lifted read are the same in both references ------------------------------------------------------------
def read_fa(path):
    out, name = {}, None
    for line in open(path):
        if line.startswith(">"):
            name = line[1:].split()[0]; out[name] = []
        elif name is not None:
            out[name].append(line.strip())
    return {k: "".join(v) for k, v in out.items()}


def exact_case(case, d):
    old, new = read_fa(os.path.join(G12, case + ".old.fa")), read_fa(os.path.join(G12, case + ".new.fa"))
    refs = [(k, len(v)) for k, v in old.items()]
    recs = [lc.rec(i, s, cig=[(20, "M")], qname="%d_%d" % (i, s)) for i, (k, v) in enumerate(old.items()) for s in range(0, len(v) - 19)]
    bam = str(d / (case + ".bam")); open(bam, "wb").write(bgzf(lc.bam_bytes("", refs, recs), 0xff00))
    return old, new, refs, recs, bam, os.path.join(G12, case + ".build.chain")


def exact_check(case, out, bed, old, new, refs, recs):
    text, new_refs, got = lc.decode(out)
    rows = open(bed).read().split("\n")[:-1]
    assert len(got) + len(rows) == len(recs)
    for g in got:
        i, s = (int(x) for x in g["qname"].split("_"))
        a, b = old[refs[i][0]][s:s + 20], new[new_refs[g["rid"]][0]][g["pos"]:g["pos"] + 20]
        assert len(b) == 20 and a.lower() == b.lower(), (case, g["qname"], g["rid"], g["pos"], a, b)
    return len(got), len(rows)


@pytest.mark.parametrize("case", ["worked", "ends", "fold", "letters", "order"])
def test_exact_chain_bases_under_a_lifted_read_are_the_same(tmp_path, case):
    old, new, refs, recs, bam, chain = exact_case(case, tmp_path)
    r, out, bed = run_lift(tmp_path, bam, chain)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    kept, rows = exact_check(case, out, bed, old, new, refs, recs)
    assert kept > len(recs) / 2 and rows > len(recs) / 20, (kept, rows, len(recs))
    v, k2, rows2 = lc.lift_all(open(chain).read(), refs, recs)
    assert kept == len(k2) and open(bed).read() == "".join(x + "\n" for x in rows2)


@pytest.mark.parametrize("case", ["minus", "minus2"])
def test_reads_under_minus_chains_all_go_to_the_bed(tmp_path, case):
    old, new, refs, recs, bam, chain = exact_case(case, tmp_path)
    r, out, bed = run_lift(tmp_path, bam, chain)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    kept, rows = exact_check(case, out, bed, old, new, refs, recs)
    assert kept == 0 and rows == len(recs) and rows > 100

"""CPU tests of `airlift-align lift --sorted --host`: the twin's order and the run store behind the command, against the rules of lift_cases.py followed by
Python's stable sort on the key (lift_sort_cases.py), and against the records the flagless `lift` writes: the CLI matrix (BGZF member size, piece size,
--sort-mem), every directed set, the header cases, equal keys spread over pieces and spills, and that `lift` without the flag still writes what the golden
g13 expects."""
import json
import os
import re

import pytest

import lift_cases as lc
import lift_sort_cases as ls
from select_cases import bgzf
from test_lift_cpu import G13, W_GUESS, run_lift

SETS = ls.self_check(W_GUESS)


def check_sorted(r, out, bed, header, refs, recs, chain_text, flagless=None):
    """the sorted output against Python, and against a flagless run's (out, bed) when given; returns the inflated stream"""
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    t = ls.truth(chain_text, refs, recs)
    stream = ls.inflate(out)
    got = ls.split_records(stream)
    assert b"".join(got) == t["packed"]                                          # byte for byte Python's records in Python's order
    text, new_refs, dec = lc.decode(out)
    tab = lc.Table(chain_text)
    assert new_refs == list(zip(tab.q_names, tab.q_sizes)) and text == ls.sorted_header(header, tab) and "SO:coordinate" in text
    assert [ls.key(dict(rid=g["rid"], pos=g["pos"])) for g in dec] == t["keys"] and t["keys"] == sorted(t["keys"])
    assert open(bed).read() == "".join(x + "\n" for x in t["rows"])
    if flagless:
        assert sorted(got) == sorted(ls.split_records(ls.inflate(flagless[0]))) and open(bed, "rb").read() == open(flagless[1], "rb").read()
    return stream


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("lift_sorted")
    chain = str(d / "directed.chain"); open(chain, "w").write(lc.CHAIN)
    big = str(d / "big.chain"); open(big, "w").write(ls.BIG_CHAIN)
    return d, {lc.CHAIN: chain, ls.BIG_CHAIN: big}


@pytest.fixture(scope="module")
def cli_case(work):
    """the matrix's input at both member sizes, and the flagless run's outputs"""
    d, chains = work
    recs = lc.directed(257) + lc.walk_sets(W_GUESS)["long"] + lc.walk_sets(W_GUESS)["cut1"]
    out = {}
    for block in (700, 0xff00):
        bam = str(d / ("cli%d.bam" % block)); open(bam, "wb").write(bgzf(lc.bam_bytes(lc.HEADER, lc.REFS, recs), block))
        fd = d / ("flagless%d" % block); fd.mkdir()
        r, o, b = run_lift(fd, bam, chains[lc.CHAIN], "--piece", "4096", AL_INFLATE_PIECE_KB=2)
        assert r.returncode == 0, r.stderr.decode()[-1500:]
        out[block] = (bam, o, b)
    return recs, out


def timing(err, what):
    m = re.search(r"(\d+) " + what, err)
    assert m, err[-1500:]
    return int(m.group(1))


@pytest.mark.parametrize("sort_mem", [2000, None])
@pytest.mark.parametrize("piece", [1000, 4096, None])
@pytest.mark.parametrize("block", [700, 0xff00])
def test_cli_matrix_on_the_host(work, cli_case, tmp_path, block, piece, sort_mem):
    d, chains = work
    recs, case = cli_case
    bam, fo, fb = case[block]
    extra = ["--sorted"] + (["--piece", str(piece)] if piece else []) + (["--sort-mem", str(sort_mem)] if sort_mem else [])
    r, out, bed = run_lift(tmp_path, bam, chains[lc.CHAIN], *extra, AL_INFLATE_PIECE_KB=2 if piece else 1024, AL_TIMING=1)
    check_sorted(r, out, bed, lc.HEADER, lc.REFS, recs, lc.CHAIN, (fo, fb))
    err = r.stderr.decode()
    assert "(host twin):" in err and "lift --sorted:" in err
    pieces, spills = timing(err, "pieces,"), timing(err, "spills")
    assert timing(err, "pieces in order") + timing(err, "pieces sorted") == pieces
    if sort_mem and piece:
        assert (pieces > 3 or block != 700) and spills >= 2, err[-600:]   # (a piece is at least one member: two members of 0xff00 bytes hold the input)
        # (2000 bytes: 8 KB of records lie in front of the 17 KB record of the "long" set, 16 KB behind it)
    if not sort_mem:
        assert spills == 0


@pytest.mark.parametrize("name", sorted(SETS))
def test_directed_sets_in_one_piece_and_in_many(work, tmp_path, name):
    d, chains = work
    chain_text, recs = SETS[name]
    bam = str(tmp_path / "in.bam"); open(bam, "wb").write(bgzf(lc.bam_bytes(lc.HEADER, lc.REFS, recs), 700))
    r, out, bed = run_lift(tmp_path, bam, chains[chain_text], "--sorted")
    one = check_sorted(r, out, bed, lc.HEADER, lc.REFS, recs, chain_text)
    r, out, bed = run_lift(tmp_path, bam, chains[chain_text], "--sorted", "--piece", "1000", "--sort-mem", "3000", AL_INFLATE_PIECE_KB=1)
    assert check_sorted(r, out, bed, lc.HEADER, lc.REFS, recs, chain_text) == one


@pytest.mark.parametrize("name", sorted(lc.HEADERS))
def test_header_says_coordinate(work, tmp_path, name):
    d, chains = work
    recs = lc.directed(40)
    bam = str(tmp_path / "h.bam"); open(bam, "wb").write(bgzf(lc.bam_bytes(lc.HEADERS[name], lc.REFS, recs), 90))
    r, out, bed = run_lift(tmp_path, bam, chains[lc.CHAIN], "--sorted")
    check_sorted(r, out, bed, lc.HEADERS[name], lc.REFS, recs, lc.CHAIN)
    text = lc.decode(out)[0]
    assert text.count("SO:coordinate") == 1 and text.count("@HD") == 1 and "SO:unsorted" not in text and "SO:queryname" not in text and text.count("@SQ") == 3
    if name == "full":
        assert text == "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:newA\tLN:12000\n@SQ\tSN:newB\tLN:3000\n@SQ\tSN:newC\tLN:700\n@PG\tID:x\tPN:x\n"
    if name in ("pg_only", "empty"):
        assert text.startswith("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:newA")
    if name == "hd_only":
        assert text.startswith("@HD\tVN:1.6\tSO:coordinate\tGO:none\n@SQ")
    if name == "sq_first":
        assert text.startswith("@SQ\tSN:newA\tLN:12000\n@SQ\tSN:newB\tLN:3000\n@SQ\tSN:newC\tLN:700\n@HD\tVN:1.6\tSO:coordinate\n@RG")


def test_without_the_flag_the_bytes_are_those_of_golden_g13(work, tmp_path):
    """`lift` without --sorted: the records, the header (SO:unsorted) and the rows the committed fixture holds, in input order"""
    exp = json.load(open(os.path.join(G13, "expected.json")))
    for case, e in sorted(exp.items()):
        r, out, bed = run_lift(tmp_path, os.path.join(G13, e["bam"]), os.path.join(G13, e["chain"]), "--piece", "4096", AL_INFLATE_PIECE_KB=2, AL_TIMING=1)
        assert r.returncode == 0 and b"lift --sorted" not in r.stderr, r.stderr.decode()[-1500:]
        text, refs, got = lc.decode(out)
        assert text == e["header"] and "SO:coordinate" not in text and [list(x) for x in refs] == e["refs"] and open(bed).read() == e["bed"]
        assert [[g[k] for k in e["fields"]] for g in got] == e["records"]
    recs = lc.directed(257); e = exp["directed257"]
    r, out, bed = run_lift(tmp_path, os.path.join(G13, e["bam"]), os.path.join(G13, e["chain"]))
    assert b"".join(ls.split_records(ls.inflate(out))) == ls.truth(lc.CHAIN, lc.REFS, recs)["unsorted"]


def test_equal_keys_keep_their_input_order_across_pieces_and_spills(work, tmp_path):
    """420 records of one key with distinct names, records of lower and of higher keys and records without a position among them, over more than four
    pieces with a spill nearly every piece: the names of the equal keys leave in input order"""
    d, chains = work
    recs = []
    for i in range(420):
        recs.append(ls.K(2500, "same%03d" % i))
        if i % 5 == 0:
            recs.append(ls.K(2300 + i, "other%d" % i))
        if i % 9 == 0:
            recs.append(ls.N("none%d" % i))
        if i % 4 == 0:
            recs.append(ls.U("gone%d" % i))
        if i % 6 == 0:
            recs.append(ls.K(5000, "high%d" % i, rid=1))
    bam = str(tmp_path / "in.bam"); open(bam, "wb").write(bgzf(lc.bam_bytes(lc.HEADER, lc.REFS, recs), 700))
    r, out, bed = run_lift(tmp_path, bam, chains[lc.CHAIN], "--sorted", "--piece", "4096", "--sort-mem", "2000", AL_INFLATE_PIECE_KB=2, AL_TIMING=1)
    check_sorted(r, out, bed, lc.HEADER, lc.REFS, recs, lc.CHAIN)
    err = r.stderr.decode()
    assert timing(err, "pieces,") >= 4 and timing(err, "spills") >= 4 and timing(err, "pieces sorted") >= 4, err[-600:]
    names = [g["qname"] for g in lc.decode(out)[2]]
    same = [n for n in names if n.startswith("same")]
    assert same == ["same%03d" % i for i in range(420)]
    assert [n for n in names if n.startswith("none")] == ["none%d" % i for i in range(0, 420, 9)] and names[-1].startswith("none")
    assert [n for n in names if n.startswith("high")] == ["high%d" % i for i in range(0, 420, 6)]


def test_usage_and_refusals(work, tmp_path):
    d, chains = work
    bam = str(tmp_path / "in.bam"); open(bam, "wb").write(bgzf(lc.bam_bytes(lc.HEADER, lc.REFS, lc.directed(10)), 700))
    r, out, bed = run_lift(tmp_path, bam, chains[lc.CHAIN], "--sorted", "extra.bam")
    assert r.returncode == 1 and b"[--sorted [--sort-mem BYTES]]" in r.stderr and b"coordinate order" in r.stderr
    blob, say = lc.malformed()["no_nul"]
    bad = str(tmp_path / "bad.bam"); open(bad, "wb").write(bgzf(blob, 700))
    for extra in ([], ["--piece", "1000", "--sort-mem", "2000"]):
        r, out, bed = run_lift(tmp_path, bad, chains[lc.CHAIN], "--sorted", *extra, AL_INFLATE_PIECE_KB=1)
        assert r.returncode == 1 and say in r.stderr.decode() and not os.path.exists(out) and not os.path.exists(bed), r.stderr.decode()[-800:]

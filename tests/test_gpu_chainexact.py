"""-m gpu tests of chain-exact.  The kernels (al_dbg_chainexact) must equal their host twin (al_dbg_chainexact_host) -- per-block counts, positions in
order, the lines after pass 1 and after pass 2, the error flag -- on the generated cases of chainexact_cases.py: every block size around the 16-byte word, the
wavefront's 64 words and the tile; all 16 x 16 start residues of the two sides; mismatches on a block's first and last base, on both sides of every tile and
word edge, on every base, on none; '+' and '-'; blocks that start at text offset 0 and end on the texts' last byte, those also fenced and poisoned in a fresh
process; pass 2 at three values of --min-region.  Then the command on the device against every g12 golden, byte for byte, and its product through
`chain-beds` and `tokens --chain`."""
import os
import subprocess
import sys

import pytest

import chainexact_cases as cx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
GOLDEN = cx.golden()


def _lib():
    import airlift_amd as A
    return A.load()


@pytest.fixture(scope="module")
def cases():
    L = _lib()
    tile = L.al_dbg_chainexact_tile()
    assert tile % 16 == 0 and tile >= 64
    out = {name: (case, M, cx.tap(L.al_dbg_chainexact_host, case, M)) for name, case, M in cx.synthetic(tile)}
    assert {"plus_sizes_edges", "minus_sizes_every", "plus_residues", "minus_residues", "plus_text_ends", "minus_text_ends", "fold_M1", "fold_M100", "fold_M5000", "random"} <= set(out)
    return out


NAMES = ["%s_%s" % (s, w) for s in ("plus", "minus") for w in ("sizes_edges", "sizes_every", "sizes_none", "residues", "text_ends")] + ["fold_M1", "fold_M100", "fold_M5000", "random"]


@pytest.mark.parametrize("name", NAMES)
def test_kernels_equal_their_twin(cases, name):
    case, M, want = cases[name]
    got = cx.tap(_lib().al_dbg_chainexact, case, M)
    for k, what in enumerate(("counts", "positions", "lines after pass 1", "lines after pass 2", "flag")):
        assert got[k] == want[k], what
    assert want[4] == 0 and (name.endswith("none") or sum(want[0]) > 0)
    if name.endswith("sizes_every"):
        assert want[0] == [b[1] if k % 2 == 0 else 1 for k, b in enumerate(case.blocks)]
    # verify stops after the counts
    cnt = cx.tap(_lib().al_dbg_chainexact, case, M, build=False)
    assert cnt == (want[0], [], [], [], 0)


def test_a_minus_block_with_an_R_raises_the_flag_and_says_nothing():
    L = _lib()
    c = cx.minus_with_an_R(L.al_dbg_chainexact_tile())
    assert cx.tap(L.al_dbg_chainexact, c) == ([0, 0], [], [], [], 1)
    assert cx.tap(L.al_dbg_chainexact, c, build=False) == ([0, 0], [], [], [], 1)


CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import airlift_amd as A
import chainexact_cases as cx
L = A.load()
for name, case, M in cx.synthetic(L.al_dbg_chainexact_tile()):
    if name.endswith("text_ends") or name == "fold_M100":
        assert cx.tap(L.al_dbg_chainexact, case, M) == cx.tap(L.al_dbg_chainexact_host, case, M), name
        print("same", name)
"""


def test_text_ends_fenced_and_poisoned_in_a_fresh_process():
    env = dict(os.environ, AL_TEST_GUARD="1", AL_TEST_POISON="170")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout.count(b"same") == 3 and b"GUARD" not in r.stderr, r.stderr.decode()[-2000:]


def _run(args, cwd, **env):
    r = subprocess.run([CLI] + args, cwd=str(cwd), capture_output=True, timeout=120, env=dict(os.environ, AL_PG_PLAIN="1", **env))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r


@pytest.mark.parametrize("case", GOLDEN, ids=[g[0] for g in GOLDEN])
def test_chain_exact_on_the_device_writes_the_scripts_bytes(case, tmp_path):
    name, p, want = case
    for mode in ("verify", "build"):
        assert _run(["chain-exact", mode, p["old"], p["new"], p["chain"]], tmp_path).stdout == want[mode], mode
    r = _run(["chain-exact", "build", "-o", "x.chain", "--device", "0", p["old"], p["new"], p["chain"]], tmp_path, AL_TIMING="1")
    assert (tmp_path / "x.chain").read_bytes() == want["build"] and b"chainexact:" in r.stderr and b"kernels" in r.stderr


def test_refused_on_the_device_as_on_the_host(tmp_path):
    seq = "ACGTTGCAAGGCTTAC" * 40; rc = cx.revcomp(seq)
    (tmp_path / "old.fa").write_text(">cA\n%s\n" % seq); (tmp_path / "new.fa").write_text(">qA\n%s\n" % (rc[:200] + "R" + rc[201:]))
    (tmp_path / "x.chain").write_text("chain 1 cA 640 + 0 600 qA 640 - 0 600 1\n300 0 0\n300\n")
    for mode in ("verify", "build"):
        r = subprocess.run([CLI, "chain-exact", mode, "old.fa", "new.fa", "x.chain"], cwd=str(tmp_path), capture_output=True, timeout=120)
        assert r.returncode == 1 and r.stdout == b"" and b"x.chain:3: a block of a '-' chain compares a new-side byte other than acgtnACGTN" in r.stderr, r.stderr


def test_the_built_chain_file_feeds_chain_beds_and_tokens_chain(tmp_path):
    p = dict((g[0], g[1]) for g in GOLDEN)["random"]
    _run(["chain-exact", "build", "-o", "exact.chain", p["old"], p["new"], p["chain"]], tmp_path)
    assert _run(["chain-exact", "verify", p["old"], p["new"], "exact.chain"], tmp_path).stdout == b"PASS VERIFICATION\n"
    beds = _run(["chain-beds", "--read-size", "100", "--max-errors", "5", "--gaps-out", "-", "exact.chain"], tmp_path).stdout
    assert beds.count(b"\n") > 50
    r = _run(["tokens", "--read-size", "100", "--skip", "50", "--chain", "exact.chain", "--max-errors", "5", "--gaps-out", "gaps.bed", "--merged-bed", "merged.bed", p["old"]], tmp_path)
    assert (tmp_path / "gaps.bed").read_bytes() == beds and (tmp_path / "merged.bed").read_bytes().count(b"\n") > 0, r.stderr.decode()[-1000:]

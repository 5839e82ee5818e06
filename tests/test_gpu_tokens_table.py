"""-m gpu tests of k_tok_setup, the kernel that sets up the tokens of `tokens --gaps-bed`: al_dbg_tokens_table over the case lists of tokens_cases.py, each
launch's window starts and fragment hashes compared element by element with the plain restatement and with the host twin (al_dbg_tokens_table_host).  The
launches (tokens_cases.ranges) start and end inside a region, on a region's first token, and span rows without tokens.  No index, no mapping."""
import ctypes as C

import numpy as np
import pytest

import tokens_cases as tc

pytestmark = pytest.mark.gpu
CASES = tc.cases()


@pytest.fixture(scope="module")
def lib():
    import airlift_amd as A
    return A.load()


def _call(f, c, t0, n, with_table):
    nr = len(c["heads"])
    names = b"".join(h + b"\0" for h in c["heads"])
    src = np.asarray(c["src"], dtype=np.uint64); ln = np.asarray(c["lens"], dtype=np.uint32)
    start = np.full(n + 1, 0xdeadbeefdeadbeef, dtype=np.uint64); hsh = np.full(n + 1, 0xdeadbeef, dtype=np.uint32)     # one guard element behind the n
    first = np.zeros(nr + 1, dtype=np.uint64); hp = np.zeros(nr + 1, dtype=np.uint32)
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    rc = f(nr, names, len(names), src.ctypes.data_as(u64p), ln.ctypes.data_as(u32p), c["R"], c["S"], c["seed"], t0, n,
           start.ctypes.data_as(u64p), hsh.ctypes.data_as(u32p), first.ctypes.data_as(u64p) if with_table else None, hp.ctypes.data_as(u32p) if with_table else None)
    assert start[n] == 0xdeadbeefdeadbeef and hsh[n] == 0xdeadbeef
    return rc, start[:n], hsh[:n], first, hp[:nr]


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_kernel_twin_and_restatement_agree(lib, c):
    first, hp, toks, _ = tc.expected(c["heads"], c["src"], c["lens"], c["R"], c["S"], c["seed"])
    assert first[-1] < 100000
    want_s = np.asarray([s for s, _ in toks], dtype=np.uint64); want_h = np.asarray([h for _, h in toks], dtype=np.uint32)
    for k, (t0, n) in enumerate(tc.ranges(first)):
        rc, s, h, ft, p = _call(lib.al_dbg_tokens_table, c, t0, n, k == 0)
        assert rc == 0
        rc2, s2, h2, ft2, p2 = _call(lib.al_dbg_tokens_table_host, c, t0, n, k == 0)
        assert rc2 == 0
        assert np.array_equal(s, want_s[t0:t0 + n]) and np.array_equal(h, want_h[t0:t0 + n]), (c["name"], t0, n)
        assert np.array_equal(s2, s) and np.array_equal(h2, h)
        if k == 0:
            assert list(ft) == first and list(p) == hp and list(ft2) == first and list(p2) == hp
    # a launch beyond the table is refused, by both
    assert _call(lib.al_dbg_tokens_table, c, first[-1], 1, False)[0] == -1 and _call(lib.al_dbg_tokens_table_host, c, 1, first[-1], False)[0] == -1


def test_the_launches_are_what_they_are_for():
    by = {c["name"]: c for c in CASES}
    first = tc.table(by["zero_runs"]["heads"], by["zero_runs"]["lens"], tc.R0, tc.S0)[0]
    rr = tc.ranges(first)
    assert first == [0, 0, 0, 0, 29, 29, 29, 30, 30, 30, 30, 30]
    assert (1, 27) in rr and (14, 16) in rr                  # inside row 3; from inside row 3 to the end
    assert (0, 30) in rr and (28, 2) in rr                   # from row 3's first token, and from its last, across the empty rows 4 and 5 onto row 6
    assert tc.runs(first, 28, 2) == [(0, 3), (1, 6)]

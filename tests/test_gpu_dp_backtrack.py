"""-m gpu: the traceback walk that takes a diagonal run in one step of the 16-lane group (d_backtrack, al_kernels_align.hip), on directed jobs
whose CIGARs have exact-match runs of every length around the group's 16 lanes, through both device taps against ksw_extd2_sse in every field
and the CIGAR.  tests/test_dp_backtrack_cpu.py checks the rule on arbitrary byte matrices; this checks the kernels."""
import numpy as np
import pytest

import dp_cases as D
import dp_tap as T

pytestmark = pytest.mark.gpu

SEED = 20250917
BAND8 = D.SR._replace(bw=8)                                     # band 13: the walk meets forced states in the middle of a run
OPTS = {"sr": D.SR, "band8": BAND8}
LMAX = 256


def planted(rng, qlen, tlen, runs):
    """A random target; the query follows it in exact-match runs whose lengths are taken from runs, an indel of 1 ... 12 bases between two of them."""
    t = rng.integers(0, 4, tlen, dtype=np.uint8)
    q = []; i = 0
    while len(q) < qlen and i < tlen:
        n = next(runs)
        q += t[i:i + n].tolist(); i += n
        k = int(rng.integers(1, 13))
        if rng.random() < 0.5:
            q += rng.integers(0, 4, k).tolist()                 # insertion to the query
        else:
            i += k                                              # deletion from it
    q = np.array(q[:qlen], dtype=np.uint8)
    if len(q) < qlen:
        q = np.concatenate([q, rng.integers(0, 4, qlen - len(q), dtype=np.uint8)])
    return t, q


def _runs(rng):
    while True:
        for n in rng.permutation(34):                           # every length 0 ... 33, again and again
            yield int(n)


def make_jobs():
    rng = np.random.default_rng(SEED)
    runs = _runs(rng)
    jobs = []
    for qlen in range(17, 97):
        t, q = planted(rng, qlen, 2 * qlen - 1, runs)
        for f in D.FLAGS_PRODUCTION:
            jobs.append(D.Job(t, q, f, "planted"))
    for tlen in (64, 128, 192, 255, 352):                       # one job per kernel instance of the stage (4, 8, 12, 16, 22 target blocks; <= 64: the LDS traceback tile)
        t, q = planted(rng, (tlen + 1) // 2, tlen, runs)
        for f in D.FLAGS_PRODUCTION:
            jobs.append(D.Job(t, q, f, "planted"))
    return jobs


JOBS = make_jobs()
_REF = {}


def reference(optname):
    if optname not in _REF:
        dp = D.ref_dp()
        _REF[optname] = [dp(OPTS[optname], j) for j in JOBS]
        m_runs = [c >> 4 for _, cig in _REF[optname] for c in cig if (c & 15) == 0]
        # (on the reference's CIGARs alone, before any device call)
        assert {n % 16 for n in m_runs} == set(range(16)), sorted({n % 16 for n in m_runs})
        assert any(n >= 32 for n in m_runs) and any(16 <= n < 32 for n in m_runs)
        cigs = [cig for _, cig in _REF[optname] if cig]
        assert any((c[0] & 15) in (1, 2) for c in cigs), "no CIGAR starts with I or D"
        assert any((c[-1] & 15) in (1, 2) for c in cigs), "no CIGAR ends with I or D"
    return _REF[optname]


def test_job_contents():
    assert sorted({len(j.query) for j in JOBS[:160]}) == list(range(17, 97))
    assert all(len(j.target) == 2 * len(j.query) - 1 for j in JOBS[:160])
    assert sorted({len(j.target) for j in JOBS[160:]}) == [64, 128, 192, 255, 352]
    for name in OPTS:
        reference(name)


@pytest.fixture(scope="module")
def small_index():
    import airlift_amd as A
    rng = np.random.default_rng(5)
    idx = A.Index(seqs=[T.text(rng.integers(0, 4, 4000))], names=[b"chr"])
    yield idx
    idx.close()


@pytest.mark.parametrize("form", ["one_cell_per_lane", "two_cells_per_lane"])
@pytest.mark.parametrize("optname", list(OPTS))
def test_ksw_tap_equals_reference(small_index, optname, form, monkeypatch):
    """al_dbg_ksw: d_ksw_reg (and its LDS traceback tile for the small jobs), d_ksw_pk with AL_DBG bit 20; both directions."""
    want = reference(optname)
    if form == "two_cells_per_lane":
        monkeypatch.setenv("AL_DBG", str(1 << 20))
    cap = max(len(c) for _, c in want) + 1
    out, cig = T.ksw_tap(small_index, OPTS[optname], JOBS, cap)
    T.compare_ksw_tap(OPTS[optname], JOBS, want, out, cig, form)


@pytest.mark.parametrize("optname", list(OPTS))
def test_stage_kernels_equal_reference(optname):
    """al_dbg_ext_dp: the align stage's kernels by class (k_ext_dp_lane, k_ext_dp<4> with the LDS tile, k_ext_dp<8 / 12 / 16 / 22> two cells per lane)."""
    want = reference(optname)
    cap = max(len(c) for _, c in want) + 1
    got, cig, _ = T.ext_dp_tap(OPTS[optname], JOBS, LMAX, cap)
    T.compare_ext_dp(OPTS[optname], JOBS, want, got, cig, optname)
    by_blocks = {(len(j.target) + 15) // 16: g["class"] for j, g in zip(JOBS[160:], got[160:])}
    assert by_blocks == {4: 5, 8: 6, 12: 7, 16: 7, 22: 7}, by_blocks  # every launch of k_ext_dp: class 5 = 4 blocks (LDS traceback tile), 6 = 8 blocks, 7 = 12 / 16 / 22 blocks by target length

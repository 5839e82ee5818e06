"""-m gpu: how k_ext_dp stages a job (d_stage_job, al_kernels_align.hip): eight bases per lane from the packed read and reference words, the pads
as constants, the packed form's selector bytes straight from the codes.  Jobs through al_dbg_ext_dp whose query starts and ends on every
residue mod 8 of the read's packed words, on both strands, in both directions, at either end of the read, with N at the edges of the 8-base
windows, compared with ksw_extd2_sse field by field."""
import numpy as np
import pytest

import dp_cases as D
import dp_tap as T

pytestmark = pytest.mark.gpu

READ_LENS = (149, 150, 151)
Q_LENS = tuple(range(1, 18)) + (63, 64, 65)


def make_jobs():
    rng = np.random.default_rng(20250918)
    jobs, reads = [], []
    for rl in READ_LENS:
        for ql in Q_LENS:
            starts = [0, rl - ql] + [16 + k for k in range(8)]              # on the read's first base, up to its last, and every residue mod 8
            for a in starts:
                for flag in D.FLAGS_PRODUCTION:
                    for rev in (0, 1):
                        n = len(jobs)
                        tl = 2 * ql - 1 + n % 3
                        t = rng.integers(0, 4, tl, dtype=np.uint8)
                        q = t[:ql].copy() if tl >= ql else np.concatenate([t, rng.integers(0, 4, ql - tl, dtype=np.uint8)])
                        sub = np.flatnonzero(rng.random(ql) < 0.04)
                        q[sub] = (q[sub] + 1) & 3
                        # position in the read (mapping orientation) of query base k: a left extension's query lies reversed in the read
                        pos = a + (ql - 1 - np.arange(ql) if flag == D.FLAG_LEFT_EXT else np.arange(ql))
                        if n % 4 == 1:                                      # N at either end of an 8-base window of the packed read (stored forward ...
                            q[(pos % 8 == 0) | (pos % 8 == 7)] = 4
                        elif n % 4 == 2:                                    # ... or reverse-complemented)
                            back = rl - 1 - pos
                            q[(back % 8 == 0) | (back % 8 == 7)] = 4
                        elif n % 4 == 3:                                    # N in the target's windows
                            m = np.arange(tl)
                            t[((m % 8 == 0) | (m % 8 == 7)) & (rng.random(tl) < 0.3)] = 4
                        jobs.append(D.Job(t, q, flag, "staging")); reads.append((rl, a, rev))
    return jobs, reads


JOBS, READS = make_jobs()
_WANT = []


def test_job_contents():
    tab = T.place(JOBS, 151, reads=READS)[2]
    assert {int(x) for x in tab[:, 4]} == set(Q_LENS)
    for kind in (0, 1):
        for rev in (0, 1):
            sel = (tab[:, 2] == kind) & (tab[:, 1] == rev)
            assert {int(x) % 8 for x in tab[sel, 3]} == set(range(8))       # qoff on every residue
            assert {int(x) % 8 for x in tab[sel, 4]} == set(range(8))       # qlen on every residue
    first = [r for j, r in zip(JOBS, READS) if r[1] == 0]; last = [r for j, r in zip(JOBS, READS) if r[1] + len(j.query) == r[0]]
    assert first and last and {r[0] for r in READS} == set(READ_LENS)
    assert any((j.query == 4).any() for j in JOBS) and any((j.target == 4).any() for j in JOBS)


@pytest.mark.parametrize("lanes", ["lane_kernels", "no_lane_kernels"])
def test_staged_jobs_equal_reference(lanes, monkeypatch):
    """Default: the small jobs take k_ext_dp_lane (staging untouched), the rest k_ext_dp.  With AL_DBG bit 29 every job takes k_ext_dp: one cell per
    lane up to 4 target blocks, two cells per lane above."""
    if not _WANT:
        dp = D.ref_dp()
        _WANT.extend(dp(D.SR, j) for j in JOBS)
    if lanes == "no_lane_kernels":
        monkeypatch.setenv("AL_DBG", str(1 << 29))                          # read when the context is created
    cap = max(len(c) for _, c in _WANT) + 1
    got, cig, _ = T.ext_dp_tap(D.SR, JOBS, 151, cap, reads=READS)
    classes = {g["class"] for g in got}
    assert (classes >= {3, 4, 5, 6, 7}) if lanes == "no_lane_kernels" else (0 in classes and 6 in classes), classes
    T.compare_ext_dp(D.SR, JOBS, _WANT, got, cig, lanes)

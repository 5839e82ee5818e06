"""CPU: the extension DP's early-exit rule evaluated every S-th anti-diagonal only (AL_DP_EXIT_STRIDE, al_dev_ksw2.h).

The rule U = max(F(r - 1), F(r), B(r)) is sound at whatever row it is evaluated, so testing it at the rows r = S - 1 (mod S) alone -- with F
accumulated in that row and the one before it, nowhere else -- must leave {max, max_t, max_q, reach_end, mqe_t if reach_end} as the full DP
computes them, and can only leave later than the test of every row does.  The DP is the numpy restatement of tests/test_dp_exit_cpu.py with
the gate added; its job generators are that file's.  This checks the rule, not the kernel (tests/test_gpu_dp_exit_stride.py does).

The 8-block class takes the rule without E3's first alternative (d_ksw_pk's EXIT == 2): it may leave only where no later row can z-drop or
have an empty band, so there zdropped must be the full run's too, whatever S is."""
import numpy as np
import pytest

from test_dp_exit_cpu import NEG, SR, _job, _row_bounds, extd as extd_every_row

STRIDES = (1, 2, 4, 8)
ROWS2 = {s: 0 for s in STRIDES}   # rows the EXIT == 2 form saved, over every job a test checked
ZD = [0, 0]                        # jobs whose full run z-drops, jobs


def extd_stride(query, target, a, b, q, e, q2, e2, w, zdrop, end_bonus, stride, form=1):
    """extd() of tests/test_dp_exit_cpu.py with the exit on and d_ksw_pk's gates: F is taken in the rows (r & (S - 1)) >= S - 2, the test runs in
    the rows (r & (S - 1)) == S - 1.  form: d_ksw_pk's EXIT (0: no exit, the full DP; 1: E1 - E3; 2: E3 without its first alternative).
    Returns (outputs the callers read, rows run, zdropped)."""
    if q2 + e2 < q + e:
        q, e, q2, e2 = q2, e2, q, e
    qlen, tlen = len(query), len(target)
    if w < 0:
        w = max(qlen, tlen)
    qe, qe2 = q + e, q2 + e2
    gap = lambda ln: min(q + e * ln, q2 + e2 * ln)   # noqa: E731
    H = np.full((tlen + 1, qlen + 1), NEG, dtype=np.int64)
    E1 = np.full_like(H, NEG); E2 = np.full_like(H, NEG); F1 = np.full_like(H, NEG); F2 = np.full_like(H, NEG)
    H[0, 0] = 0
    for t in range(tlen):
        H[t + 1, 0] = -gap(t + 1); E1[t + 1, 0] = -(q + e * (t + 1)); E2[t + 1, 0] = -(q2 + e2 * (t + 1))
    for i in range(qlen):
        H[0, i + 1] = -gap(i + 1); F1[0, i + 1] = -(q + e * (i + 1)); F2[0, i + 1] = -(q2 + e2 * (i + 1))
    qa, ta = np.asarray(query), np.asarray(target)
    mx, max_t, max_q, mqe, mqe_t, zdropped = 0, -1, -1, NEG, -1, False
    ex_on = form != 0 and a + max(b, 1) <= qe
    no_empty = tlen - 1 <= ((qlen + tlen - 2 + w) >> 1)
    xs = stride - 1
    f_prev, rows = NEG, 0
    for r in range(qlen + tlen - 1):
        st, en = _row_bounds(r, qlen, tlen, w)
        if st > en:
            zdropped = True
            break
        rows = r + 1
        ts = np.arange(st, en + 1); is_ = r - ts
        qb, tb = qa[is_], ta[ts]
        sc = np.where((qb > 3) | (tb > 3), -1, np.where(qb == tb, a, -b))
        e1 = np.maximum(H[ts, is_ + 1] - qe, E1[ts, is_ + 1] - e); e2_ = np.maximum(H[ts, is_ + 1] - qe2, E2[ts, is_ + 1] - e2)
        f1 = np.maximum(H[ts + 1, is_] - qe, F1[ts + 1, is_] - e); f2 = np.maximum(H[ts + 1, is_] - qe2, F2[ts + 1, is_] - e2)
        h = np.maximum.reduce([H[ts, is_] + sc, e1, e2_, f1, f2])
        H[ts + 1, is_ + 1] = h; E1[ts + 1, is_ + 1] = e1; E2[ts + 1, is_ + 1] = e2_; F1[ts + 1, is_ + 1] = f1; F2[ts + 1, is_ + 1] = f2
        if r - st == qlen - 1 and h[0] > mqe:
            mqe, mqe_t = int(h[0]), st
        k = int(np.argmax(h)); row_h, row_t = int(h[k]), st + k
        if row_h > mx:
            mx, max_t, max_q = row_h, row_t, r - row_t
        elif row_t >= max_t and r - row_t >= max_q:
            tl, ql = row_t - max_t, (r - row_t) - max_q
            if zdrop >= 0 and mx - row_h > zdrop + abs(tl - ql) * e2:
                zdropped = True
                break
        if ex_on and r >= qlen - 1 and (r & xs) >= xs - 1:                  # acc_row
            f_row = int(np.max(h + a * (qlen - 1 - is_)))
            if r >= qlen and (r & xs) == xs:                                # the test row: f_prev is F(r - 1), taken in the row before
                assert r - 1 >= qlen - 1 and ((r - 1) & xs) >= xs - 1
                t1 = r + 1
                bnd = a * (1 + min(qlen - 1, tlen - 2 - r)) - gap(t1) if t1 <= tlen - 1 and t1 <= w else NEG
                U = max(f_row, f_prev, bnd)
                wok = ((r - w) >> 1) <= r - qlen
                c1 = U <= mx
                c2 = U <= mqe or (U + end_bonus <= mx and mqe + end_bonus <= mx)
                kq = qlen - 1 - max_q
                c3 = (form != 2 and mqe + end_bonus <= mx) or (no_empty and (zdrop < 0 or (max_t >= 0 and kq * max(b, 1) + q2 <= zdrop and max_t + kq <= tlen - 1
                                                                          and r + 2 - qlen - max_t - kq >= 0)))
                if wok and c1 and c2 and c3:
                    break
            f_prev = f_row
    reach = (not zdropped) and mqe + end_bonus > mx
    return (mx, max_t, max_q, reach, mqe_t if reach else None), rows, zdropped


def _check(query, target, w=151, **kw):
    p = dict(SR); p.update(kw)
    full, n_full = extd_every_row(query, target, w=w, use_exit=False, **p)
    every, n_every = extd_every_row(query, target, w=w, use_exit=True, **p)
    same, n_same, zd_full = extd_stride(query, target, w=w, stride=1, form=0, **p)
    assert (same, n_same) == (full, n_full)                                 # (form 0 is that file's full DP: its zdropped is the full run's)
    rows = {}; rows2 = {}
    for s in STRIDES:
        got, rows[s], _ = extd_stride(query, target, w=w, stride=s, **p)
        assert got == full, (s, p, w, list(query), list(target), full, got)
        got2, rows2[s], zd2 = extd_stride(query, target, w=w, stride=s, form=2, **p)
        assert got2 == full and zd2 == zd_full, (s, p, w, list(query), list(target), full, zd_full, got2, zd2)
        assert rows[s] <= rows2[s] <= n_full                                # the stricter form leaves no sooner
        if rows2[s] < n_full:
            assert (rows2[s] - 1) & (s - 1) == s - 1
        ROWS2[s] += n_full - rows2[s]; ZD[0] += zd_full; ZD[1] += 1
        assert n_every <= rows[s] <= n_full
        if rows[s] < n_full:                                                # left early: at a test row, at most S - 1 rows behind the first row the rule holds at ...
            assert (rows[s] - 1) & (s - 1) == s - 1
    assert rows[1] == n_every                                               # S = 1 is the rule as it was
    return rows, n_full


def test_stride_random_jobs():
    rng = np.random.default_rng(21)
    saved = {s: 0 for s in STRIDES}; total = 0
    for _ in range(60):
        qlen = int(rng.integers(1, 120))
        q, t = _job(rng, qlen, p_sub=float(rng.choice([0.0, 0.01, 0.05, 0.2])), p_indel=float(rng.choice([0.0, 0.01, 0.05])),
                    tl_factor=float(rng.choice([0.3, 1.0, 2.0, 3.0])))
        rows, nf = _check(q, t)
        total += nf
        for s in STRIDES:
            saved[s] += nf - rows[s]
    assert saved[8] > 0.08 * total                                          # the rule still fires on ordinary jobs
    assert saved[1] >= saved[2] >= saved[4] >= saved[8]


def test_stride_form2_fires_and_keeps_zdropped():
    """The EXIT == 2 form on jobs that z-drop and jobs that do not (checked in _check: outputs and zdropped equal the full run's at every S):
    it must still save rows, and the set must hold both kinds."""
    rng = np.random.default_rng(26)
    for s in STRIDES:
        ROWS2[s] = 0
    ZD[0] = ZD[1] = 0; total = 0
    for k in range(48):
        qlen = int(rng.integers(20, 100))
        q, t = _job(rng, qlen, p_sub=float(rng.choice([0.0, 0.02])), p_indel=float(rng.choice([0.0, 0.02])), tl_factor=2.0)
        if k % 3 == 0:                                                      # a clipped flank: the query's tail is random, the full run z-drops
            q = np.concatenate([q[:qlen // 2], rng.integers(0, 4, qlen - qlen // 2)])
        total += _check(q, t, zdrop=int(rng.choice([30, 100])))[1]
    assert 0 < ZD[0] < ZD[1], ZD
    assert ROWS2[8] > 0.05 * total, (ROWS2, total)
    assert ROWS2[1] >= ROWS2[2] >= ROWS2[4] >= ROWS2[8]


def flank_jobs(qlens=range(65, 81), seed=22):
    """Perfect flanks of 65 ... 80 bases against 2 qlen - 1: the rule first holds at row 2 qlen - 2, an even row whatever qlen is.  The same
    flanks with one target base deleted five bases before the query's end move it to an odd row: together every residue mod 8."""
    rng = np.random.default_rng(seed)
    out = []
    for qlen in qlens:
        query = rng.integers(0, 4, qlen)
        target = np.concatenate([query, rng.integers(0, 4, qlen - 1)])
        out.append((query, target))
        out.append((query, np.concatenate([np.delete(target, qlen - 5), rng.integers(0, 4, 1)])))
    return out


def test_stride_exit_row_on_every_residue():
    first = set()
    for k, (query, target) in enumerate(flank_jobs()):
        assert len(target) == 2 * len(query) - 1
        rows, nf = _check(query, target)
        assert rows[1] < nf
        if k % 2 == 0:
            assert rows[1] == 2 * len(query) - 1
        first.add((rows[1] - 1) & 7)
        for s in STRIDES:
            assert rows[s] - rows[1] <= s                                   # (once the rule holds here it keeps holding: S - 1 rows late at the most, and one more for r >= qlen)
    assert first == set(range(8)), first


def test_stride_form2_exit_row_on_every_residue():
    """Flanks of the 8-block class (target of 97 ... 127 bases): the EXIT == 2 form leaves them too, its first exit row on every residue mod 8."""
    first = set()
    for query, target in flank_jobs(range(49, 65), 27):
        p = dict(SR)
        full, nf = extd_every_row(query, target, w=151, use_exit=False, **p)
        rows = {s: extd_stride(query, target, w=151, stride=s, form=2, **p) for s in STRIDES}
        assert rows[1][1] < nf
        first.add((rows[1][1] - 1) & 7)
        for s in STRIDES:
            assert rows[s][0] == full and not rows[s][2] and rows[s][1] - rows[1][1] <= s
    assert first == set(range(8)), first


@pytest.mark.parametrize("tail", ["random", "repeat"])
def test_stride_tandem_repeats_past_the_end(tail):
    rng = np.random.default_rng(23)
    for _ in range(15):
        _check(*_job(rng, int(rng.integers(5, 100)), tail=tail))


@pytest.mark.parametrize("w", [3, 10, 40])
@pytest.mark.parametrize("tl_factor", [0.5, 4.0])
def test_stride_lengths_and_bands(tl_factor, w):
    rng = np.random.default_rng(24 + w)
    for _ in range(6):
        _check(*_job(rng, int(rng.integers(1, 80)), tl_factor=tl_factor, p_indel=0.02), w=w)


@pytest.mark.parametrize("zdrop", [-1, 5, 30])
@pytest.mark.parametrize("end_bonus", [0, 10, 200])
def test_stride_zdrop_and_end_bonus(zdrop, end_bonus):
    rng = np.random.default_rng(25 + zdrop + end_bonus)
    for _ in range(6):
        _check(*_job(rng, int(rng.integers(5, 80)), p_sub=float(rng.choice([0.02, 0.2])), p_indel=0.03, n_frac=0.03), zdrop=zdrop, end_bonus=end_bonus)

"""CPU: the early-exit rule of the extension DP (al_dev_ksw2.h) on a restatement of ksw2's dual-affine extension DP in
anti-diagonal order, with its band, max / mqe / z-drop / end-bonus rules.  Stopping at the first row where E1-E3 hold must leave every
output an extension job's caller reads ({max, max_t, max_q, reach_end, mqe_t if reach_end}) as the full run computes it.  This checks
the rule, not the kernel (tests/test_gpu_dp_exit.py checks the kernel)."""
import numpy as np
import pytest

NEG = -(1 << 30)


def _row_bounds(r, qlen, tlen, w):
    st, en = 0, tlen - 1
    st = max(st, r - qlen + 1)
    en = min(en, r)
    st = max(st, (r - w + 1) >> 1)
    en = min(en, (r + w) >> 1)
    return st, en


def extd(query, target, a, b, q, e, q2, e2, w, zdrop, end_bonus, use_exit):
    """Returns (outputs the callers read, rows run).  query / target: int arrays of bases 0-3, 4 = N."""
    if q2 + e2 < q + e:
        q, e, q2, e2 = q2, e2, q, e
    qlen, tlen = len(query), len(target)
    if w < 0:
        w = max(qlen, tlen)
    qe, qe2 = q + e, q2 + e2
    gap = lambda ln: min(q + e * ln, q2 + e2 * ln)   # noqa: E731  (ln >= 1)
    # H, E (target gaps), F (query gaps) per cell; row -1 / column -1 are the boundary
    H = np.full((tlen + 1, qlen + 1), NEG, dtype=np.int64)    # index [t + 1, i + 1]
    E1 = np.full_like(H, NEG); E2 = np.full_like(H, NEG); F1 = np.full_like(H, NEG); F2 = np.full_like(H, NEG)
    H[0, 0] = 0
    for t in range(tlen):
        H[t + 1, 0] = -gap(t + 1); E1[t + 1, 0] = -(q + e * (t + 1)); E2[t + 1, 0] = -(q2 + e2 * (t + 1))
    for i in range(qlen):
        H[0, i + 1] = -gap(i + 1); F1[0, i + 1] = -(q + e * (i + 1)); F2[0, i + 1] = -(q2 + e2 * (i + 1))
    qa, ta = np.asarray(query), np.asarray(target)
    mx, max_t, max_q, mqe, mqe_t, zdropped = 0, -1, -1, NEG, -1, False
    ex_on = use_exit and a + max(b, 1) <= qe
    no_empty = tlen - 1 <= ((qlen + tlen - 2 + w) >> 1)
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
        # ---- the exit rule, as d_ksw_pk evaluates it
        if ex_on and r >= qlen - 1:
            f_row = int(np.max(h + a * (qlen - 1 - is_)))
            if r >= qlen:
                t1 = r + 1
                bnd = a * (1 + min(qlen - 1, tlen - 2 - r)) - gap(t1) if t1 <= tlen - 1 and t1 <= w else NEG
                U = max(f_row, f_prev, bnd)
                wok = ((r - w) >> 1) <= r - qlen
                c1 = U <= mx
                c2 = U <= mqe or (U + end_bonus <= mx and mqe + end_bonus <= mx)
                kq = qlen - 1 - max_q
                c3 = mqe + end_bonus <= mx or (no_empty and (zdrop < 0 or (max_t >= 0 and kq * max(b, 1) + q2 <= zdrop and max_t + kq <= tlen - 1
                                                                          and r + 2 - qlen - max_t - kq >= 0)))
                if wok and c1 and c2 and c3:
                    break
            f_prev = f_row
    reach = (not zdropped) and mqe + end_bonus > mx
    return (mx, max_t, max_q, reach, mqe_t if reach else None), rows


SR = dict(a=2, b=8, q=12, e=2, q2=24, e2=1, zdrop=100, end_bonus=10)


def _check(query, target, w=151, **kw):
    p = dict(SR); p.update(kw)
    full, n_full = extd(query, target, w=w, use_exit=False, **p)
    ex, n_ex = extd(query, target, w=w, use_exit=True, **p)
    assert ex == full, (p, w, list(query), list(target), full, ex)
    return n_ex, n_full


def _mutate(rng, s, p_sub=0.02, p_indel=0.0):
    out = []
    for x in s:
        u = rng.random()
        if u < p_indel / 2:
            continue
        if u < p_indel:
            out.append(int(rng.integers(4)))
        out.append(int(rng.integers(4)) if rng.random() < p_sub else int(x))
    return np.array(out, dtype=np.int64)


def _job(rng, qlen, tail="random", p_sub=0.02, p_indel=0.0, tl_factor=2.0, n_frac=0.0):
    query = rng.integers(0, 4, qlen)
    if n_frac:
        query[rng.random(qlen) < n_frac] = 4
    core = _mutate(rng, query, p_sub, p_indel)
    tlen = max(1, int(qlen * tl_factor))
    if tail == "repeat":
        unit = query[-min(qlen, 1 + int(rng.integers(6))):]
        extra = np.resize(unit, max(0, tlen - len(core)))
    else:
        extra = rng.integers(0, 4, max(0, tlen - len(core)))
    target = np.concatenate([core, extra])[:tlen]
    return query, target


def test_exit_rule_random_jobs():
    rng = np.random.default_rng(1)
    saved = total = 0
    for _ in range(150):
        qlen = int(rng.integers(1, 120))
        q, t = _job(rng, qlen, p_sub=float(rng.choice([0.0, 0.01, 0.05, 0.2])), p_indel=float(rng.choice([0.0, 0.01, 0.05])),
                    tl_factor=float(rng.choice([0.3, 1.0, 2.0, 3.0])))
        ne, nf = _check(q, t)
        saved += nf - ne; total += nf
    assert saved > 0.1 * total                              # (the rule does fire on ordinary jobs)


@pytest.mark.parametrize("tail", ["random", "repeat"])
def test_exit_rule_tandem_repeats_past_the_end(tail):
    rng = np.random.default_rng(2)
    for _ in range(40):
        _check(*_job(rng, int(rng.integers(5, 100)), tail=tail))


def test_exit_rule_errors_in_the_last_bases():
    rng = np.random.default_rng(3)
    for k in range(1, 6):
        for _ in range(12):
            qlen = int(rng.integers(10, 100))
            query = rng.integers(0, 4, qlen)
            core = query.copy()
            pos = qlen - 1 - rng.integers(0, k, size=2)
            core[pos] = (core[pos] + 1) % 4                                        # mismatches in the last k bases
            if rng.random() < 0.5:                                                 # or an indel there
                j = qlen - k
                core = np.concatenate([core[:j], rng.integers(0, 4, int(rng.integers(1, 4))), core[j:]]) if rng.random() < 0.5 else np.delete(core, j)
            target = np.concatenate([core, rng.integers(0, 4, qlen)])
            _check(query, target)


def test_exit_rule_n_bases():
    rng = np.random.default_rng(4)
    for _ in range(30):
        q, t = _job(rng, int(rng.integers(5, 90)), n_frac=0.1)
        t = t.copy(); t[rng.random(len(t)) < 0.05] = 4
        _check(q, t)


@pytest.mark.parametrize("tl_factor", [0.05, 0.5, 4.0, 6.0])
@pytest.mark.parametrize("w", [3, 10, 40, 151])
def test_exit_rule_lengths_and_bands(tl_factor, w):
    """tlen far from qlen either way, bands that clip rows on both sides and go empty."""
    rng = np.random.default_rng(5 + w)
    for _ in range(8):
        _check(*_job(rng, int(rng.integers(1, 80)), tl_factor=tl_factor, p_indel=0.02), w=w)


def test_exit_rule_qlen_one():
    rng = np.random.default_rng(6)
    for _ in range(30):
        _check(rng.integers(0, 5, 1), rng.integers(0, 5, int(rng.integers(1, 20))))


@pytest.mark.parametrize("zdrop", [-1, 0, 5, 20, 30])
@pytest.mark.parametrize("end_bonus", [0, 10, 200])
def test_exit_rule_zdrop_and_end_bonus(zdrop, end_bonus):
    rng = np.random.default_rng(7 + zdrop + end_bonus)
    for _ in range(12):
        _check(*_job(rng, int(rng.integers(5, 80)), p_sub=float(rng.choice([0.02, 0.2])), p_indel=0.03), zdrop=zdrop, end_bonus=end_bonus)


@pytest.mark.parametrize("gaps", [dict(q=4, e=2, q2=24, e2=1, a=2, b=4), dict(q=24, e=1, q2=12, e2=2), dict(q=6, e=2, q2=6, e2=2),
                                  dict(a=1, b=4, q=6, e=1, q2=26, e2=1), dict(a=5, b=12, q=6, e=2, q2=20, e2=1)],
                         ids=["ont", "swapped", "single", "asm", "rule_off"])
def test_exit_rule_gap_models(gaps):
    rng = np.random.default_rng(8)
    for _ in range(20):
        _check(*_job(rng, int(rng.integers(3, 80)), p_sub=0.05, p_indel=0.03), **gaps)

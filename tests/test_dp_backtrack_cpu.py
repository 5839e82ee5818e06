"""CPU: the traceback walk of the extension DP (d_backtrack, al_kernels_align.hip) in its two forms, restated in Python.

ksw_backtrack (ksw2.h:119-151, is_rot = 1, no introns) walks one cell per step.  d_backtrack takes a diagonal run in one step of the 16-lane
group: in state 0, lane k looks at cell (i - k, j - k) and the leading lanes that see a match there (inside the matrix, not forced, low three
bits 0) are taken at once.  The walk accepts any byte matrix, so both restatements must give the same CIGAR on random bytes (all 256 values,
garbage outside the band included) from every end cell, and on matrices with planted diagonals of every length around 16 and 32.
This checks the rule, not the kernel (tests/test_gpu_dp_backtrack.py checks the kernel)."""
import numpy as np
import pytest

LENS = (1, 2, 15, 16, 17, 33, 40)
BANDS = (3, 8, 151)
GW = 16


def _row_bounds(r, qlen, tlen, w):
    st, en = 0, tlen - 1
    st = max(st, r - qlen + 1)
    en = min(en, r)
    st = max(st, (r - w + 1) >> 1)
    en = min(en, (r + w) >> 1)
    return st, en


def _blocks(r, qlen, tlen, w):
    """off[r], off_end[r] of ksw_extd2_sse, recomputed from r as d_backtrack does."""
    st, en = _row_bounds(r, qlen, tlen, w)
    return st // 16 * 16, (en + 16) // 16 * 16 - 1


def n_col(qlen, tlen, w):
    n = min(qlen, tlen)
    return ((min(n, w + 1) + 15) // 16 + 1) * 16


def _push(cig, op, ln):
    if cig and cig[-1][0] == op:
        cig[-1][1] += ln
    else:
        cig.append([op, ln])


def _finish(cig, i, j, is_rev):
    if i >= 0:
        _push(cig, 2, i + 1)
    if j >= 0:
        _push(cig, 1, j + 1)
    out = [(ln << 4) | op for op, ln in cig]
    return tuple(out if is_rev else out[::-1])


def _single(p, nc, qlen, tlen, w, i, j, state, cig):
    """One step of the serial walk from cell (i, j); returns the new (i, j, state) and whether the step was a plain match."""
    r = i + j
    off, off_end = _blocks(r, qlen, tlen, w)
    force = -1
    if i < off:
        force = 2
    if i > off_end:
        force = 1
    tmp = int(p[r * nc + i - off]) if force < 0 else 0
    plain = state == 0 and force < 0 and (tmp & 7) == 0
    if state == 0:
        state = tmp & 7
    elif not (tmp >> (state + 2)) & 1:
        state = 0
    if state == 0:
        state = tmp & 7
    if force >= 0:
        state = force
    if state == 0:
        _push(cig, 0, 1); i -= 1; j -= 1
    elif state in (1, 3):
        _push(cig, 2, 1); i -= 1
    else:
        _push(cig, 1, 1); j -= 1
    return i, j, state, plain


def walk_serial(p, qlen, tlen, w, is_rev, i0, j0, runs=None):
    """The serial walk; runs (optional list) receives the length of every maximal run of plain matches."""
    nc = n_col(qlen, tlen, w)
    i, j, state, cig, run = i0, j0, 0, [], 0
    while i >= 0 and j >= 0:
        i, j, state, plain = _single(p, nc, qlen, tlen, w, i, j, state, cig)
        if plain:
            run += 1
        else:
            if runs is not None and run:
                runs.append(run)
            run = 0
    if runs is not None and run:
        runs.append(run)
    return _finish(cig, i, j, is_rev)


def walk_runs(p, qlen, tlen, w, is_rev, i0, j0):
    """The run-of-16 form: every lane's load is unconditional, at index 0 where its cell cannot be part of the run."""
    nc = n_col(qlen, tlen, w)
    i, j, state, cig = i0, j0, 0, []
    while i >= 0 and j >= 0:
        if state == 0:
            n = 0
            verdicts = []
            for k in range(GW):
                ik, jk = i - k, j - k
                off, off_end = _blocks(ik + jk, qlen, tlen, w)
                inside = ik >= 0 and jk >= 0 and off <= ik <= off_end
                idx = (ik + jk) * nc + ik - off if inside else 0
                assert 0 <= idx < len(p)                                    # the load of every lane stays inside the traceback area
                verdicts.append(inside and (int(p[idx]) & 7) == 0)
            while n < GW and verdicts[n]:                                   # trailing ones of the group's ballot
                n += 1
            if n:
                _push(cig, 0, n); i -= n; j -= n
            if n == GW:
                continue
            if i < 0 or j < 0:
                break
        i, j, state, _ = _single(p, nc, qlen, tlen, w, i, j, state, cig)
    return _finish(cig, i, j, is_rev)


def end_cells(qlen, tlen):
    """Every cell of the last query row and of the last target column, as (i0, j0) = (target, query) index."""
    return [(i, qlen - 1) for i in range(tlen)] + [(tlen - 1, j) for j in range(qlen - 1)]


def random_matrix(rng, qlen, tlen, w, p_zero=0.0):
    m = rng.integers(0, 256, size=(qlen + tlen - 1) * n_col(qlen, tlen, w), dtype=np.uint8)
    if p_zero:
        m[rng.random(len(m)) < p_zero] &= 0xf8                              # longer runs of state 0 than chance gives
    return m


@pytest.mark.parametrize("w", BANDS)
@pytest.mark.parametrize("is_rev", [0, 1])
def test_run_form_equals_serial_walk_on_random_bytes(w, is_rev):
    rng = np.random.default_rng([7, w, is_rev])
    walks = 0
    for qlen in LENS:
        for tlen in LENS:
            for p_zero in (0.0, 0.9):
                p = random_matrix(rng, qlen, tlen, w, p_zero)
                for (i0, j0) in end_cells(qlen, tlen):
                    a = walk_serial(p, qlen, tlen, w, is_rev, i0, j0)
                    b = walk_runs(p, qlen, tlen, w, is_rev, i0, j0)
                    assert a == b, (qlen, tlen, w, is_rev, i0, j0, a, b)
                    walks += 1
    assert walks == 2 * sum(q + t - 1 for q in LENS for t in LENS)


def test_all_byte_values_are_used():
    rng = np.random.default_rng(8)
    seen = set()
    for qlen in LENS:
        for tlen in LENS:
            seen |= set(random_matrix(rng, qlen, tlen, 151).tolist())
    assert len(seen) == 256


@pytest.mark.parametrize("w", BANDS)
def test_planted_diagonals_of_every_length(w):
    """Diagonals of 0 ... 40 plain matches ending in a cell that is no match, from the last cell of a 40 x 40 matrix and from cells off the main
    diagonal (where a narrow band forces a state in the middle of the run)."""
    qlen = tlen = 40
    nc = n_col(qlen, tlen, w)
    rng = np.random.default_rng([9, w])
    seen = set()
    for shift in (0, 2, 7):                                                 # the diagonal i - j = shift
        for length in range(0, 41):
            p = random_matrix(rng, qlen, tlen, w)
            p |= 1 + (p & 1)                                                # no plain match anywhere (low bits 1 ... 3) ...
            i0, j0 = tlen - 1, qlen - 1 - shift
            for k in range(length):                                         # ... but along the planted diagonal, where the cell is stored
                i, j = i0 - k, j0 - k
                if i < 0 or j < 0:
                    break
                off, off_end = _blocks(i + j, qlen, tlen, w)
                if off <= i <= off_end:
                    p[(i + j) * nc + i - off] &= 0xf8
            for is_rev in (0, 1):
                runs = []
                a = walk_serial(p, qlen, tlen, w, is_rev, i0, j0, runs)
                assert a == walk_runs(p, qlen, tlen, w, is_rev, i0, j0), (w, shift, length, is_rev)
                seen |= set(runs)
                if shift == 0:
                    assert (runs[0] if runs else 0) == length               # the main diagonal is inside every band
    for need in (15, 16, 17, 31, 32, 33):
        assert need in seen, (need, sorted(seen))

"""Directed anchor sets for the chaining stage, shared by tests/test_chain_oracle_cpu.py and tests/test_gpu_chain_directed.py, and the ctypes
view of the reference function they are compared with (mm_chain_dp, chain.c:22-162, compiled as oracle/_ref/libchainref.so by oracle/Makefile).

A fragment is (qlens, anchors, tie, label, k): the mates' read lengths, its anchors as an (n, 2) uint64 array in the order the chain stage sees
them (ascending x; anchors of equal x keep the order they were generated in), whether two anchors have equal x, a name, and the k-mer length
its anchors span (one per fragment: the stage's anchors all have the index's k; 0 for a fragment without anchors: any).
    x = rev << 63 | rid << 32 | pos          y = seg << 48 | span << 32 | qpos
Everything is deterministic: every family's generator is seeded by its name, so a label names one fragment for good."""
import ctypes as C
import os
import subprocess
import zlib
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

Opt = namedtuple("Opt", "bw max_gap max_gap_ref max_frag_len min_cnt min_chain_score max_chain_skip max_chain_iter k")
SR = Opt(100, 100, -1, 800, 2, 25, 25, 5000, 21)               # -x sr (options.c)
OPTION_SETS = {
    "sr": SR,
    "bw500": SR._replace(bw=500),
    "skip0": SR._replace(max_chain_skip=0),
    "skip5": SR._replace(max_chain_skip=5),
    "skip6": SR._replace(max_chain_skip=6),                    # below the tile kernel's bound (tiles_ok: max_chain_skip >= 7) ...
    "skip7": SR._replace(max_chain_skip=7),                    # ... and on it
    "iter128": SR._replace(max_chain_iter=128),                # the LDS forms' bound (lds_ok: max_chain_iter >= 128) ...
    "iter127": SR._replace(max_chain_iter=127),                # ... and below it
    "min_cnt1": SR._replace(min_cnt=1, min_chain_score=15),    # one anchor may be a chain: lmin < 2, no tile kernel
    "min_cnt3_sc40": SR._replace(min_cnt=3, min_chain_score=40),
    "max_gap40000": SR._replace(max_gap=40000),                # max_dist_x > 0x7fff: outside the 16-bit window-relative positions
    "k15": SR._replace(k=15),
    "k28": SR._replace(k=28),
}
SPANS = (15, 19, 21, 25, 28)
SEG_SIZES = (1, 2, 3, 8, 9, 16, 17, 24, 25, 32, 33, 40, 41, 48, 49, 64, 65, 80, 81, 96, 97, 128, 129, 1024, 1025)
FRAG_SIZES = (0, 1, 2, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2049, 8193)
END_COUNTS = (63, 64, 65)                                      # chain ends in one segment (CT_NU_CAP)
CHAIN_COUNTS = (40, 63, 64, 65, 127, 128, 129)                 # chains of a fragment with tied starts (the reference's sort is stable up to 64; AL_ORDER_BLOCK)
PE = (150, 150)

Frag = namedtuple("Frag", "qlens anchors tie label k")                # k: the span of its anchors, i.e. the k of the index it would come from


def chain_gaps(o, qlens):
    """(max_chain_gap_ref, max_chain_gap_qry) of a fragment under -x sr: map.c:341-351, what the kernels derive from frag_meta."""
    qs = sum(qlens)
    qry = qs if qs > o.max_gap else o.max_gap
    if o.max_gap_ref > 0:
        ref = o.max_gap_ref
    elif o.max_frag_len > 0:
        ref = max(o.max_frag_len - qs, o.max_gap)
    else:
        ref = o.max_gap
    return ref, qry


def _frag(qlens, pts, label):
    """pts: rows of (rev, rid, pos, seg, span, qpos)."""
    a = np.array(pts, dtype=np.int64).reshape(-1, 6).astype(np.uint64)
    x = a[:, 0] << np.uint64(63) | a[:, 1] << np.uint64(32) | a[:, 2]
    y = a[:, 3] << np.uint64(48) | a[:, 4] << np.uint64(32) | a[:, 5]
    assert len(a) == 0 or int(a[:, 2].max()) < 1 << 31, label
    order = np.argsort(x, kind="stable")
    xy = np.ascontiguousarray(np.stack([x[order], y[order]], axis=1))
    tie = bool(len(x) > 1 and (xy[1:, 0] == xy[:-1, 0]).any())
    assert len(qlens) in (1, 2) and (len(xy) == 0 or int(a[:, 3].max()) < len(qlens)), label
    spans = set(a[:, 4].tolist())
    assert len(spans) <= 1, label
    return Frag(tuple(qlens), xy, tie, label, int(spans.pop()) if spans else 0)


def _rng(name):
    return np.random.default_rng([20250301, zlib.crc32(name.encode())])


def segments(o, f):
    """Lengths of the independent chaining problems of a fragment: cut wherever two neighbours are more than max_dist_x apart (chain.c:51)."""
    n = len(f.anchors)
    if n == 0:
        return []
    x = f.anchors[:, 0]; mdx = np.uint64(chain_gaps(o, f.qlens)[0])
    cut = np.flatnonzero(x[1:] > x[:-1] + mdx) + 1
    return np.diff(np.concatenate([[0], cut, [n]])).tolist()


# ---- building blocks ---------------------------------------------------------------------------------------------------------------
def _run(pos, q, n, step, seg, span, rev=0, rid=0):
    """n anchors on one diagonal, step bases apart."""
    return [(rev, rid, pos + i * step, seg, span, q + i * step) for i in range(n)]


def _bridge(qlens, span, dr, dq, seg_j, seg_i, label, pos=100000, q0=5, n=3, q_lim=4096):
    """Three anchors ten bases apart, the pair under test (dr, dq), three more: one chain if the pair may be joined, two if not.  The query
    positions are free of the read lengths (max_dist_y >= qlen_sum: a same-mate dq on it lies outside any real read) but stay below q_lim."""
    if q0 + 10 * (n - 1) + dq + 10 * (n - 1) >= q_lim:
        return None
    a = _run(pos, q0, n, 10, seg_j, span)
    pj, qj = pos + 10 * (n - 1), q0 + 10 * (n - 1)
    return _frag(qlens, a + _run(pj + dr, qj + dq, n, 10, seg_i, span), label)


def _dense_segment(g, n, pos, qs, n_segs, span, distinct, max_step=3, q_hi=None):
    """n anchors whose neighbours are at most max_step bases apart (one segment under every option set), random query positions and mates."""
    steps = g.integers(1 if distinct else 0, max_step + 1, size=n)
    p = pos + np.cumsum(steps)
    q = g.integers(0, q_hi or qs, size=n)
    s = g.integers(0, n_segs, size=n)
    return [(0, 0, int(p[i]), int(s[i]), span, int(q[i])) for i in range(n)], int(p[-1]) if n else pos


def _colinear_segment(g, n, pos, qs, n_segs, span):
    """Like _dense_segment, but most anchors lie on a few diagonals, so that long chains with side branches form."""
    steps = g.integers(1, 4, size=n); p = pos + np.cumsum(steps)
    diag = g.integers(0, 4, size=n) * 7
    q = (p - pos) // 2 % max(qs - 40, 1) + diag
    noise = g.random(n) < 0.2
    q = np.where(noise, g.integers(0, qs, size=n), q) % qs
    s = g.integers(0, n_segs, size=n) if n_segs > 1 else np.zeros(n, dtype=np.int64)
    return [(0, 0, int(p[i]), int(s[i]), span, int(q[i])) for i in range(n)], int(p[-1]) if n else pos


# ---- the families --------------------------------------------------------------------------------------------------------------------
def pair_sweep(o, spans):
    """Two anchors (and two with a decoy) at every dd in 0 ... bw + 1 on both sides, same mate and other mate; dr == 0; dq around the span."""
    out = []
    base = 30
    dds = list(range(0, o.bw + 2))
    for span in spans:
        for other in (0, 1):
            # (a band wider than the reads: one read for the same mate, so that dr may pass max_dist_y, and short mates, so that max_dist_x is wide)
            qlens = PE if o.bw + 40 < PE[0] else (100, 100) if other else (150,)
            for side in ("r", "q"):
                for dd in dds:
                    dr, dq = (base + dd, base) if side == "r" else (base, base + dd)
                    pj = (0, 0, 5000, 0, span, 3)
                    pi = (0, 0, 5000 + dr, other, span, 3 + dq)
                    lab = "span%d %s dd%d side_%s" % (span, "other" if other else "same", dd, side)
                    out.append(_frag(qlens, [pj, pi], "pair " + lab))
                    out.append(_frag(qlens, [pj, pi, (0, 0, 5000 + dr + 3, 0, span, 4)], "pair+decoy " + lab))
            for dq in (1, span - 1, span, span + 1):            # dr == 0: skipped for the same mate, + 1 for the other
                out.append(_frag(qlens, [(0, 0, 7000, 0, span, 3), (0, 0, 7000, other, span, 3 + dq)], "pair dr0 span%d other%d dq%d" % (span, other, dq)))
                out.append(_frag(qlens, [(0, 0, 7000, 0, span, 3), (0, 0, 7000, other, span, 3 + dq), (0, 0, 7000 + span, other, span, 3 + dq + span)], "pair+1 dr0 span%d other%d dq%d" % (span, other, dq)))
            for dq in (0, 1, span - 1, span, span + 1):         # min_d against q_span
                for ex in (0, 2):
                    out.append(_frag(qlens, [(0, 0, 9000, 0, span, 3), (0, 0, 9000 + dq + ex, other, span, 3 + dq)], "pair min_d span%d other%d dq%d dr+%d" % (span, other, dq, ex)))
                    out.append(_frag(qlens, [(0, 0, 9000, 0, span, 3), (0, 0, 9000 + dq, other, span, 3 + dq + ex)], "pair min_d span%d other%d dr%d dq+%d" % (span, other, dq, ex)))
    return out


def range_boundaries(o):
    out = []
    span = o.k
    q_lim = 4096 if max(o.max_gap, o.max_frag_len, o.max_gap_ref) <= 0x7fff else 1 << 30    # (12-bit query positions in the compact rows of the LDS forms)
    for qlens in (PE, (300,), (2000,), (350, 350), (350, 351), (349, 350)):   # (max_frag_len - qlen_sum on, below and above max_gap)
        mdx, mdy = chain_gaps(o, qlens)
        two = len(qlens) > 1
        T = []
        for e in (0, 1):
            T.append((mdy + e, mdy + e, 0, 0, "same dq=mdy+%d" % e))
            T.append((max(mdx + e - 5, 1), mdx + e, 0, 1 if two else 0, "dq=mdx+%d" % e))
            T.append((mdx + e, max(mdx + e - 5, 1), 0, 1 if two else 0, "dr=mdx+%d" % e))
            T.append((mdy + e, max(mdy + e - 50, 1), 0, 0, "same dr=mdy+%d" % e))
            T.append((30 + o.bw + e, 30, 0, 0, "same dd=bw+%d dr>dq" % e))
            T.append((30, 30 + o.bw + e, 0, 0, "same dd=bw+%d dq>dr" % e))
            if two:
                T.append((30 + o.bw + e, 30, 0, 1, "other dd=bw+%d dr>dq" % e))
                T.append((mdy + e, max(mdy + e - 50, 1), 0, 1, "other dr=mdy+%d" % e))
        for dr, dq, sj, si, lab in T:
            out.append(_bridge(qlens, span, dr, dq, sj, si, "range %s: %s (dr %d dq %d)" % (qlens, lab, dr, dq), q_lim=q_lim))
    return out


def window_cut(o):
    out = []
    span = o.k
    for qlens in (PE, (300,)):
        mdx, _ = chain_gaps(o, qlens)
        other = len(qlens) - 1
        for e in (-1, 0, 1):                                    # neighbour gaps around max_dist_x: only a larger gap cuts
            for si in {0, other}:
                out.append(_bridge(qlens, span, mdx + e, 12, 0, si, "cut %s gap=mdx%+d mate%d" % (qlens, e, si)))
            # ... with an anchor in between, so that the window's start and the neighbour gap differ
            a = _run(50000, 5, 3, 10, 0, span); pj = 50020
            mid = [(0, 0, pj + mdx // 2, 0, span, 3)]
            out.append(_frag(qlens, a + mid + _run(pj + mdx + e, 37, 3, 10, other, span), "cut %s window=mdx%+d over a stepping stone" % (qlens, e)))
        # strand / contig changes whose 32-bit position is smaller or equal
        for (rv, rd, p2, lab) in ((0, 1, 400, "contig, smaller pos"), (0, 1, 60020, "contig, equal pos"), (1, 0, 400, "strand, smaller pos"), (1, 0, 60025, "strand, pos + 5"), (1, 1, 60020, "both, equal pos")):
            out.append(_frag(qlens, _run(60000, 5, 3, 10, 0, span) + _run(p2, 40, 3, 10, 0, span, rev=rv, rid=rd), "cut %s change of %s" % (qlens, lab)))
        # equal low 16 position bits, 65536 apart (and a little more)
        for d in (65536, 65536 + 7, 2 * 65536, 65536 - 1):
            out.append(_frag(qlens, _run(70000, 5, 3, 10, 0, span) + _run(70020 + d, 32, 3, 10, 0, span), "cut %s neighbours %d apart" % (qlens, d)))
        out.append(_frag(qlens, _run(70000, 5, 3, 10, 0, span) + _run(70020 + 65536, 32, 3, 10, 0, span) + _run(70040 + 2 * 65536 + 7, 60, 3, 10, 0, span), "cut %s three runs 65536 apart" % (qlens,)))
        # positions up to 2^31 - 1, the largest a seed hit can have (map.c:163-198 keeps 31 bits), and chains across the 16-bit wrap of the position
        top = (1 << 31) - 1
        for p in (top - 50, 65536 - 25, (1 << 30) + 65536 - 11):
            out.append(_frag(qlens, _run(p, 5, 6, 10, 0, span), "cut %s chain from pos %d" % (qlens, p)))
        for p in (top - (60 + 2 * mdx + 1), 65536 - 25 - mdx, (1 << 30) + 65536 - 30):
            out.append(_frag(qlens, _run(p, 5, 3, 10, 0, span) + _run(p + 20 + mdx, 37, 3, 10, other, span) + _run(p + 40 + 2 * mdx + 1, 70, 3, 10, other, span), "cut %s runs from pos %d, gaps mdx and mdx+1" % (qlens, p)))
    return out


def sizes(o):
    out = []
    g = _rng("sizes")
    span = o.k
    mdx, _ = chain_gaps(o, PE)
    qs = sum(PE)
    for s in SEG_SIZES:                                         # one dense segment of every size, alone and between two small ones
        a = _run(1000, 5, min(s, 4), 10, 0, span) + (_colinear_segment(g, s - 4, 1040, qs, 2, span)[0] if s > 4 else [])
        out.append(_frag(PE, a, "size segment %d" % s))
        b0, e0 = _colinear_segment(g, 5, 1000, qs, 2, span)
        b1, e1 = _colinear_segment(g, s, e0 + mdx + 1, qs, 2, span)
        b2, _ = _colinear_segment(g, 4, e1 + mdx + 2, qs, 2, span)
        out.append(_frag(PE, b0 + b1 + b2, "size segment %d between two" % s))
    for n in FRAG_SIZES:
        a = _run(1000, 5, n, 10, 0, span) if n <= 8 else _dense_segment(g, n, 1000, qs, 2, span, True)[0]
        out.append(_frag(PE, a, "size fragment %d, one segment" % n))
        pts, pos, left, i = [], 1000, n, 0
        while left > 0:                                         # many small segments: the class edges in turn
            s = min(left, SEG_SIZES[(i * 5 + n) % 16]); i += 1
            a, end = _colinear_segment(g, s, pos, qs, 2, span) if i % 2 else _dense_segment(g, s, pos, qs, 2, span, True)
            pts += a; left -= s; pos = end + mdx + 1 + int(g.integers(0, 40))
        out.append(_frag(PE, pts, "size fragment %d, small segments" % n))
    # a tile of 1024 anchors must end on a segment boundary: segments of 100 (the 11th straddles anchor 1024), of 7, of 127 and 128
    for s, n in ((100, 1500), (7, 1100), (127, 1300), (128, 1300), (9, 2100)):
        pts, pos = [], 1000
        for i in range(0, n, s):
            a, end = _colinear_segment(g, min(s, n - i), pos, qs, 2, span)
            pts += a; pos = end + mdx + 1
        out.append(_frag(PE, pts, "size tile slice: %d anchors in segments of %d" % (n, s)))
    return out


DENSE_SIZES = (40, 64, 100, 128, 129, 200, 2000, 3000)


def _diag_cloud(g, n, width, n_diag, noise, qstep, qlens, span, distinct):
    """n anchors within width reference bases on n_diag diagonals along which the query advances qstep times slower than the reference (every
    step costs a little, many predecessors score alike and long chains run side by side), a share of them anywhere: the rows have far more than
    max_skip predecessors, and whether chain.c:74-81 breaks off before the best one decides the result."""
    qs = sum(qlens)
    p = np.sort(g.choice(width, size=n, replace=False) if distinct else g.integers(0, width, size=n)) + 2000
    q = ((p - 2000) // qstep + g.integers(0, n_diag, size=n) * 11) % qs
    q = np.where(g.random(n) < noise, g.integers(0, qs, size=n), q)
    sg = g.integers(0, len(qlens), size=n)
    return [(0, 0, int(p[i]), int(sg[i]), span, int(q[i])) for i in range(n)]


def dense(o):
    """Many anchors within a few hundred reference bases: every row has far more than max_skip predecessors."""
    out = []
    g = _rng("dense")
    span = o.k
    shapes = [(300, 300, 6, 0.3)] * 14 + [(300, 420, 6, 0.3)] * 6 + [(500, 400, 6, 0.4)] * 8 + [(1000, 400, 8, 0.4)] * 4 + [(n, max(120, n * 2 // 5), 6, 0.35) for n in DENSE_SIZES]
    for i, (n, width, nd, noise) in enumerate(shapes):
        qlens = PE if i % 3 else (300,)
        distinct = n <= width and i % 2 == 0
        out.append(_frag(qlens, _diag_cloud(g, n, width, nd, noise, 3, qlens, span, distinct), "dense %d anchors in %d bases #%d%s" % (n, width, i, "" if distinct else " with equal x")))
    for i in range(6):                                          # and without any structure
        qlens = PE if i % 2 else (300,)
        a, _ = _dense_segment(g, 300, 2000, 300, len(qlens), span, i < 3, max_step=2)
        out.append(_frag(qlens, a, "dense 300 random anchors #%d" % i))
    return out


def chain_ends(o):
    out = []
    span = o.k
    g = _rng("ends")
    # peak before the end: a tight run, then an anchor that costs more than it brings
    for dq, dd in ((3, 80), (1, 60), (5, 95)):
        out.append(_frag(PE, _run(1000, 5, 4, 10, 0, span) + [(0, 0, 1030 + dq + dd, 0, span, 35 + dq)], "ends peak before end dq%d dd%d" % (dq, dd)))
        out.append(_frag(PE, _run(1000, 5, 4, 10, 0, span) + [(0, 0, 1030 + dq + dd, 0, span, 35 + dq), (0, 0, 1030 + dq + dd + 2, 0, span, 35 + dq + 2)], "ends peak two before end dq%d dd%d" % (dq, dd)))
    # a branch off a longer chain: the trunk on one diagonal; the longer chain leaves it for a diagonal 90 bases off and goes on; the branch goes
    # on 15 bases off the other way (105 > bw between the two: neither reaches the other).  The branch's backtrack runs into the trunk, which
    # the longer chain has taken; what the branch adds is swept over min_chain_score by its last step
    for nb in (2, 3, 4):
        for last in range(1, span + 1):
            trunk = _run(1000, 5, 5, 10, 0, span) + _run(1140, 55, 8, 10, 0, span)
            br = [(0, 0, 1040 + 12 * (i + 1), 0, span, 45 + 15 + 12 * (i + 1)) for i in range(nb - 1)]
            br.append((0, 0, br[-1][2] + last, 0, span, br[-1][5] + last))
            out.append(_frag(PE, trunk + br, "ends branch of %d, last step %d" % (nb, last)))
    # lone chains of 1 ... 4 anchors, the last step swept: v around min_chain_score, counts around min_cnt
    for m in (1, 2, 3, 4):
        for last in range(1, span + 2):
            a = _run(1000, 5, m - 1, 10, 0, span) if m > 1 else []
            p, q = (1000 + (m - 2) * 10 + last, 5 + (m - 2) * 10 + last) if m > 1 else (1000, 5)
            out.append(_frag(PE, a + [(0, 0, p, 0, span, q)], "ends lone chain of %d, last step %d" % (m, last)))
            if m == 1:
                break
    # E chain ends in one segment: pairs whose query positions descend, so that no pair reaches another
    for E in END_COUNTS + (20,):
        m = max(2, o.min_cnt)
        qlens = ((m * span + 6) * (E + 2),)
        pts = []
        for e in range(E):
            pts += _run(1000 + 30 * e, (m * span + 6) * (E - e), m, span, 0, span)
        out.append(_frag(qlens, pts, "ends %d chain ends in one segment" % E))
    # fragments that keep no chain, between fragments that do
    keep, _ = _colinear_segment(g, 30, 1000, 300, 2, span)
    for lab, a in (("two far apart", [(0, 0, 1000, 0, span, 5), (0, 0, 9000, 0, span, 50)]),
                   ("scattered", [(0, 0, 1000 + 997 * i, i & 1, span, (i * 37) % 290) for i in range(40)]),
                   ("descending q", [(0, 0, 1000 + 2 * i, 0, span, 290 - i) for i in range(200)]),
                   ("one anchor", [(0, 0, 1000, 0, span, 5)]), ("no anchors", [])):
        out.append(_frag(PE, keep, "ends kept (before: %s)" % lab))
        out.append(_frag(PE, a, "ends nothing kept: %s" % lab))
    out.append(_frag(PE, keep, "ends kept (last)"))
    return out


def order(o):
    """Two or more chains that start at equal x: the reference's radix_sort_128x decides (stable up to 64 chains, not above)."""
    out = []
    span = o.k
    g = _rng("order")
    for i in range(60):                                         # positions snapped to multiples of 8: ties in nearly every fragment
        n = 400
        p = np.sort(g.integers(0, 150, size=n)) * 8 + 3000
        qlens = PE if i % 2 else (300,)
        a = [(0, 0, int(p[j]), int(g.integers(0, len(qlens))), span, int(g.integers(0, sum(qlens)))) for j in range(n)]
        out.append(_frag(qlens, a, "order snapped #%d" % i))
    # an exact number of chains: pairs whose query positions descend; every third pair starts where its neighbour starts; groups of per_seg
    # chains per segment (one segment: more chain ends than the serial sorts take)
    m = max(2, o.min_cnt)
    for E in CHAIN_COUNTS:
        for per_seg in (16, 1000):
            qs = min(4095, (span + 2) * (E + 3) + m * span)
            mdx, _ = chain_gaps(o, (qs,))
            pts, pos = [], 1000
            for e in range(E):
                if e % 3 != 1:
                    pos += 30
                if e and e % per_seg == 0:
                    pos += mdx + 1
                pts += _run(pos, (span + 2) * (E - e), m, span, 0, span)
            out.append(_frag((qs,), pts, "order %d chains, %s per segment, tied starts" % (E, per_seg if per_seg < 1000 else "all")))
    return out


def row_limits(o):
    out = []
    span = o.k
    g = _rng("rows")
    for qlens in ((4095,), (2048, 2048)):                       # qlen_sum 4095: the last value the 12-bit rows hold; 4096: the whole batch leaves the LDS forms
        qs = sum(qlens)
        out.append(_frag(qlens, _run(1000, qs - 60, 6, 10, len(qlens) - 1, span) + [(0, 0, 1060, len(qlens) - 1, span, qs - 1)], "rows %s chain up to qpos %d" % (qlens, qs - 1)))
        for n in (2, 40, 129, 300, 1100):
            a, _ = _dense_segment(g, n, 5000, qs, len(qlens), span, n != 300, q_hi=None)
            out.append(_frag(qlens, a, "rows %s dense %d" % (qlens, n)))
            a, _ = _colinear_segment(g, n, 5000, qs, len(qlens), span)
            out.append(_frag(qlens, a, "rows %s colinear %d" % (qlens, n)))
    return out


_CACHE = {}


def cases(optname):
    """The list of one option set (computed once per process).  The pair sweep runs over every span under `sr`, over the set's own k elsewhere."""
    if optname not in _CACHE:
        o = OPTION_SETS[optname]
        out = pair_sweep(o, SPANS if optname == "sr" else (o.k,))
        out += range_boundaries(o) + window_cut(o) + sizes(o) + dense(o) + chain_ends(o) + order(o) + row_limits(o)
        out = [f for f in out if f is not None]
        assert len({f.label for f in out}) == len(out)
        _CACHE[optname] = out
    return _CACHE[optname]


def describe(optname, f, limit=48):
    o = OPTION_SETS[optname]
    mdx, mdy = chain_gaps(o, f.qlens)
    a = f.anchors
    rows = ["    %s%d:%d seg%d span%d q%d" % ("-" if int(x) >> 63 else "+", int(x) >> 32 & 0x7fffffff, int(x) & 0xffffffff, int(y) >> 48 & 0xff, int(y) >> 32 & 0xff, int(y) & 0xffffffff) for x, y in a[:limit]]
    return "option set %s %s\n  fragment '%s': reads %s (max_dist_x %d, max_dist_y %d), %d anchors%s, segments %s\n%s%s" % (
        optname, tuple(o), f.label, f.qlens, mdx, mdy, len(a), " (equal x)" if f.tie else "", segments(o, f)[:24], "\n".join(rows), "\n    ..." if len(a) > limit else "")


def chains_str(u, ch, limit=6):
    out, k = [], 0
    for i, w in enumerate(u[:limit]):
        n = int(w) & 0xffffffff
        out.append("[score %d, %d anchors from %d:%d q%d]" % (int(w) >> 32, n, int(ch[k, 0]) >> 32 & 0x7fffffff, int(ch[k, 0]) & 0xffffffff, int(ch[k, 1]) & 0xffffffff))
        k += n
    return "%d chains: %s%s" % (len(u), " ".join(out), " ..." if len(u) > limit else "")


# ---- the reference and the oracle ----------------------------------------------------------------------------------------------------
class _Chain:
    """mm_chain_dp(max_dist_x, max_dist_y, bw, max_skip, max_iter, min_cnt, min_sc, is_cdna, n_segs, n, a, &n_u, &u, km) with km = NULL, or
    o_chain_dp (no is_cdna, no km).  a is handed over in libc memory (the function frees it); what it returns is freed here."""

    def __init__(self, lib, fn, ref):
        self.f = getattr(lib, fn); self.f.restype = C.c_void_p; self.ref = ref
        self.f.argtypes = [C.c_int] * 7 + ([C.c_int] if ref else []) + [C.c_int, C.c_int64, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p)] + ([C.c_void_p] if ref else [])
        libc = C.CDLL(None)
        self.malloc = libc.malloc; self.malloc.restype = C.c_void_p; self.malloc.argtypes = [C.c_size_t]
        self.free = libc.free; self.free.restype = None; self.free.argtypes = [C.c_void_p]

    def __call__(self, o, f, max_skip=None, max_iter=None):
        """(u as a uint64 array in the order returned, the chained anchors as an (m, 2) uint64 array)."""
        n = len(f.anchors); mdx, mdy = chain_gaps(o, f.qlens)
        a = None
        if n:
            a = self.malloc(n * 16); C.memmove(a, f.anchors.ctypes.data, n * 16)
        nu = C.c_int(0); u = C.c_void_p()
        args = [mdx, mdy, o.bw, o.max_chain_skip if max_skip is None else max_skip, o.max_chain_iter if max_iter is None else max_iter, o.min_cnt, o.min_chain_score]
        args += ([0] if self.ref else []) + [len(f.qlens), n, a, C.byref(nu), C.byref(u)] + ([None] if self.ref else [])
        b = self.f(*args)
        k = nu.value
        uu = np.frombuffer(C.string_at(u.value, 8 * k), dtype=np.uint64) if k else np.zeros(0, dtype=np.uint64)
        m = int((uu & np.uint64(0xffffffff)).sum())
        ch = np.frombuffer(C.string_at(b, 16 * m), dtype=np.uint64).reshape(-1, 2) if m else np.zeros((0, 2), dtype=np.uint64)
        if b:
            self.free(b)
        if u.value:
            self.free(u.value)
        return uu, ch


def ref_chain():
    """mm_chain_dp of the reference; the library is built from the reference's sources where they lie, or is the one that came with the tree."""
    p = os.path.join(ROOT, "oracle", "_ref", "libchainref.so")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "_ref/libchainref.so"], check=False, capture_output=True)
    if not os.path.exists(p):
        raise RuntimeError("oracle/_ref/libchainref.so is missing and the reference's sources are not here to build it from")
    return _Chain(C.CDLL(p), "mm_chain_dp", True)


def oracle_chain():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libal_oracle.so"], check=True, capture_output=True)
    return _Chain(C.CDLL(os.path.join(ROOT, "oracle", "libal_oracle.so")), "o_chain_dp", False)


def tied_starts(u, ch):
    """Whether two chains of a result start at equal x."""
    if len(u) < 2:
        return False
    first = np.concatenate([[0], np.cumsum((u & np.uint64(0xffffffff)).astype(np.int64))[:-1]])
    x = ch[first, 0]
    return len(np.unique(x)) < len(x)

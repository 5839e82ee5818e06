"""Directed cases for the extension DP, shared by tests/test_dp_oracle_cpu.py and tests/test_gpu_dp_directed.py, and the ctypes view of the
reference DP they are compared with (ksw_extd2_sse, compiled as oracle/_ref/libksw2ref.so by oracle/Makefile).

A job is (target, query, flag) as passed to ksw: nt4 codes 0..4, already reversed for left extensions.  Everything is deterministic: every
job's generator is seeded by (shape, kind), so a failure message's (tlen, qlen, kind, flag) names one job for good."""
import ctypes as C
import os
import subprocess
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EZ_RIGHT, EZ_EXTZ_ONLY, EZ_REV_CIGAR = 0x02, 0x40, 0x80
FLAG_RIGHT_EXT = EZ_EXTZ_ONLY                                  # right extension (align.c:760-771)
FLAG_LEFT_EXT = EZ_EXTZ_ONLY | EZ_RIGHT | EZ_REV_CIGAR         # left extension (align.c:694-704)
FLAGS_PRODUCTION = (FLAG_RIGHT_EXT, FLAG_LEFT_EXT)
FLAGS_CORE = (0, EZ_RIGHT)                                     # the core re-alignment: end_bonus = -1, ez->score matters
FLAGS = FLAGS_PRODUCTION + FLAGS_CORE
KSW_NEG_INF = -0x40000000

Opt = namedtuple("Opt", "a b q e q2 e2 sc_ambi zdrop bw end_bonus")
SR = Opt(2, 8, 12, 2, 24, 1, 1, 100, 100, 10)
OPTION_SETS = {
    "sr": SR,
    "z25_r8": SR._replace(zdrop=25, bw=8),                     # -z 25 -r 8: z-drop inside the band, the band clips both sides
    "end_bonus0": SR._replace(end_bonus=0),
    "end_bonus60": SR._replace(end_bonus=60),
    "B12": SR._replace(b=12),
    "O6_26_E2_1": SR._replace(q=6, e=2, q2=26, e2=1),
    "A2B4_O4_24_E2_1": Opt(2, 4, 4, 2, 24, 1, 1, 100, 100, 10),  # another gap model under which the early exit's precondition a + b <= q + e holds (O6_26_E2_1: it does not)
    "swap": SR._replace(q=24, e=1, q2=12, e2=2),               # q + e > q2 + e2: the DP swaps the two gap models
    "a16_gap64": Opt(16, 16, 40, 23, 62, 2, 1, 400, 100, 10),  # the two-cells-per-lane form's limits: a, b <= 16, q2 + e2 <= 64 (and the sum of both <= 127)
    "ambi2": SR._replace(sc_ambi=2),                           # outside that form's precondition (score of an N != -1; "swap" is outside it too) ...
    "a17": SR._replace(a=17),                                  # ... and a > 16: both must take the one-cell form
}
PK_OK = {k: k not in ("swap", "ambi2", "a17") for k in OPTION_SETS}     # which sets meet the two-cells-per-lane form's precondition (d_pk_ok)

T_LENS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 351, 352, 353, 511, 512, 513, 1023, 1024)
Q_LENS = (1, 2, 63, 64, 65, 160, 161, 255, 256, 257, 511, 512)
TMAX, QMAX = 1024, 512                                         # the largest window the extension stage's tiles hold

Job = namedtuple("Job", "target query flag kind")              # target, query: uint8 nt4 arrays


def shapes():
    """(tlen, qlen) pairs: every target length with a query as long and one half as long (tlen ~ 2 qlen - 1: how k_ext_prep sizes a flank),
    every query length with such targets and a shorter one, queries longer than target + band, and the edges of the lane-per-job class."""
    s = []
    for t in T_LENS:
        s += [(t, min(t, QMAX)), (t, max(1, (t + 1) // 2))]
    for q in Q_LENS:
        s += [(min(2 * q - 1, TMAX), q), (q, q), (max(1, q - 10), q)]
    for t in (1, 16, 17, 100, 200):
        s.append((t, min(QMAX, 2 * t + 20)))
    s += [(1, 64), (TMAX, 1), (300, 1), (TMAX, QMAX), (16, 64), (16, 65), (32, 64), (32, 65), (33, 64), (17, 64), (64, 64), (352, 256), (352, 257), (353, 256),
          (513, 256), (528, 250), (600, 300), (700, 504), (1000, 500), (1024, 504),     # the LDS-row class with the reads of a batch (<= 256, <= 504 bases)
          (200, 3), (340, 20)]                                                          # short queries on long targets
    out, seen = [], set()
    for x in s:
        if x not in seen:
            seen.add(x); out.append(x)
    return out


def _rand(rng, n):
    return rng.integers(0, 4, size=n, dtype=np.uint8)


def _sub(rng, s, pos):
    s = s.copy()
    for p in pos:
        s[p] = (s[p] + rng.integers(1, 4)) & 3 if s[p] < 4 else 0
    return s


def _fit(rng, s, n):
    """s cut, or continued with random bases, to n."""
    return s[:n] if len(s) >= n else np.concatenate([s, _rand(rng, n - len(s))])


def _dense(rng, t, qlen):
    """~8 % substitutions and an indel of 1 ... 30 bases about every 60."""
    out, i = [], 0
    while i < len(t) and len(out) < qlen:
        r = rng.random()
        if r < 0.08:
            out.append((int(t[i]) + int(rng.integers(1, 4))) & 3); i += 1
        elif r < 0.088:
            i += int(rng.integers(1, 31))                       # deletion from the query
        elif r < 0.096:
            out += [int(x) for x in _rand(rng, int(rng.integers(1, 31)))]
        else:
            out.append(int(t[i])); i += 1
    return _fit(rng, np.array(out[:qlen], dtype=np.uint8), qlen)


def _tandem(rng, tlen, qlen, period, ins):
    """A tandem repeat behind a short random head; the query has one unit more (ins) or one less in the middle of it."""
    head = _rand(rng, tlen // 8)
    unit = _rand(rng, period)
    if period > 1 and len(set(unit.tolist())) == 1:
        unit[0] = (unit[0] + 1) & 3
    t = np.concatenate([head, np.tile(unit, tlen // period + 2)])[:tlen]
    cut = len(head) + (min(tlen, qlen) - len(head)) // 2 // period * period
    q = np.concatenate([t[:cut], unit, t[cut:]]) if ins else np.concatenate([t[:cut], t[cut + period:]])
    return t, _fit(rng, q, qlen)


def _with_n(rng, s, frac):
    s = s.copy()
    s[rng.random(len(s)) < frac] = 4
    return s


def _kinds():
    k = {}
    k["identity"] = lambda g, T, Q: (lambda t: (t, _fit(g, t, Q)))(_rand(g, T))
    k["sparse_sub"] = lambda g, T, Q: (lambda t: (t, _sub(g, _fit(g, t, Q), np.flatnonzero(g.random(Q) < 0.02))))(_rand(g, T))
    k["dense_sub_indel"] = lambda g, T, Q: (lambda t: (t, _dense(g, t, Q)))(_rand(g, T))
    for n in (1, 3, 5):
        k["err_last%d" % n] = lambda g, T, Q, n=n: (lambda t: (t, _sub(g, _fit(g, t, Q), [max(0, Q - n)])))(_rand(g, T))
    for n in (1, 5):
        k["err_first%d" % n] = lambda g, T, Q, n=n: (lambda t: (t, _sub(g, _fit(g, t, Q), [min(Q - 1, n - 1)])))(_rand(g, T))
    k["half_then_unrelated"] = lambda g, T, Q: (lambda t: (t, np.concatenate([_fit(g, t, Q)[:Q // 2], _rand(g, Q - Q // 2)])))(_rand(g, T))   # a clipped flank
    k["unrelated"] = lambda g, T, Q: (_rand(g, T), _rand(g, Q))                                                                    # z-drop
    for p in (1, 2, 3, 7):
        k["tandem%d_ins" % p] = lambda g, T, Q, p=p: _tandem(g, T, Q, p, True)
        k["tandem%d_del" % p] = lambda g, T, Q, p=p: _tandem(g, T, Q, p, False)
    k["n5_target"] = lambda g, T, Q: (lambda t: (_with_n(g, t, 0.05), _fit(g, t, Q)))(_rand(g, T))
    k["n5_query"] = lambda g, T, Q: (lambda t: (t, _with_n(g, _fit(g, t, Q), 0.05)))(_rand(g, T))
    k["n5_both"] = lambda g, T, Q: (lambda t: (_with_n(g, t, 0.05), _with_n(g, _fit(g, t, Q), 0.05)))(_rand(g, T))
    k["all_n"] = lambda g, T, Q: (np.full(T, 4, np.uint8), np.full(Q, 4, np.uint8))
    return k


KINDS = _kinds()
KIND_NAMES = tuple(KINDS)


def make_pair(tlen, qlen, kind):
    """(target, query) of one case; seeded by the case alone."""
    g = np.random.default_rng([20240607, tlen, qlen, KIND_NAMES.index(kind)])
    t, q = KINDS[kind](g, tlen, qlen)
    t = np.ascontiguousarray(t, dtype=np.uint8); q = np.ascontiguousarray(q, dtype=np.uint8)
    assert len(t) == tlen and len(q) == qlen, (kind, tlen, qlen, len(t), len(q))
    return t, q


def cases(flags=FLAGS, max_t=TMAX, max_q=QMAX):
    """Every shape x kind x flag, as a list of Job."""
    out = []
    for (T, Q) in shapes():
        if T > max_t or Q > max_q:
            continue
        for kind in KIND_NAMES:
            t, q = make_pair(T, Q, kind)
            for f in flags:
                out.append(Job(t, q, f, kind))
    return out


def oversize_job():
    """The one job above the al_dbg_ksw tap's 1024 x 512 limit: it must be refused (n_cigar == -1), not run."""
    t, q = make_pair(1025, 10, "identity")
    return Job(t, q, FLAG_RIGHT_EXT, "identity")


def describe(optname, job):
    return "option set %s %s: tlen %d qlen %d flag 0x%x kind %s\n  target %s\n  query  %s" % (
        optname, tuple(OPTION_SETS[optname]), len(job.target), len(job.query), job.flag, job.kind,
        "".join("ACGTN"[c] for c in job.target), "".join("ACGTN"[c] for c in job.query))


# ---- the reference DP ----------------------------------------------------------------------------------------------------------------
class KswExtz(C.Structure):                                     # ksw_extz_t, ksw2.h
    _fields_ = [("max_zd", C.c_uint32), ("max_q", C.c_int), ("max_t", C.c_int), ("mqe", C.c_int), ("mqe_t", C.c_int), ("mte", C.c_int), ("mte_q", C.c_int),
                ("score", C.c_int), ("m_cigar", C.c_int), ("n_cigar", C.c_int), ("reach_end", C.c_int), ("cigar", C.POINTER(C.c_uint32))]


class OKsw(C.Structure):                                        # oksw_t, oracle/al_oracle.h
    _fields_ = [("max", C.c_uint32), ("zdropped", C.c_uint32), ("max_q", C.c_int), ("max_t", C.c_int), ("mqe", C.c_int), ("mqe_t", C.c_int), ("mte", C.c_int), ("mte_q", C.c_int),
                ("score", C.c_int), ("m_cigar", C.c_int), ("n_cigar", C.c_int), ("reach_end", C.c_int), ("cigar", C.POINTER(C.c_uint32))]


FIELDS = ("max", "zdropped", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q", "score", "reach_end")
_KSW_ARGS = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int8, C.c_void_p, C.c_int8, C.c_int8, C.c_int8, C.c_int8, C.c_int, C.c_int, C.c_int, C.c_int]


def simple_mat(o):
    """ksw_gen_simple_mat(5, ...) (align.c:9-22)."""
    a, b, amb = abs(o.a), -abs(o.b), -abs(o.sc_ambi)
    m = np.full((5, 5), b, dtype=np.int8)
    for i in range(4):
        m[i, i] = a
    m[4, :] = amb; m[:, 4] = amb
    return np.ascontiguousarray(m)


def band(o):
    return int(o.bw * 1.5 + 1.)                                # align.c:580


def end_bonus(o, flag):
    return o.end_bonus if flag & EZ_EXTZ_ONLY else -1          # align.c: extensions pass opt->end_bonus, the core re-alignment -1


class _Dp:
    def __init__(self, lib, fn, st, km):
        self.f = getattr(lib, fn); self.f.restype = None; self.f.argtypes = ([C.c_void_p] if km else []) + _KSW_ARGS + [C.POINTER(st)]
        self.st, self.km = st, km
        self.free = C.CDLL(None).free; self.free.argtypes = [C.c_void_p]; self.free.restype = None

    def __call__(self, o, job):
        """One call; returns ({field: value}, cigar as a tuple of words)."""
        ez = self.st(); mat = simple_mat(o)
        a = (len(job.query), job.query.ctypes.data, len(job.target), job.target.ctypes.data, 5, mat.ctypes.data, o.q, o.e, o.q2, o.e2, band(o), o.zdrop, end_bonus(o, job.flag), job.flag, C.byref(ez))
        self.f(*((None,) + a if self.km else a))
        if self.km:
            r = {"max": ez.max_zd & 0x7fffffff, "zdropped": ez.max_zd >> 31}
        else:
            r = {"max": ez.max, "zdropped": ez.zdropped}
        for k in FIELDS[2:]:
            r[k] = getattr(ez, k)
        cig = tuple(ez.cigar[i] for i in range(ez.n_cigar))
        if ez.cigar:
            self.free(C.cast(ez.cigar, C.c_void_p))
        return r, cig


def ref_dp():
    """ksw_extd2_sse of the reference; the library is built from the reference's sources where they lie, or is the one that came with the tree."""
    p = os.path.join(ROOT, "oracle", "_ref", "libksw2ref.so")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "_ref/libksw2ref.so"], check=False, capture_output=True)
    if not os.path.exists(p):
        raise RuntimeError("oracle/_ref/libksw2ref.so is missing and the reference's sources are not here to build it from")
    return _Dp(C.CDLL(p), "ksw_extd2_sse", KswExtz, True)


def oracle_dp():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libal_oracle.so"], check=True, capture_output=True)
    return _Dp(C.CDLL(os.path.join(ROOT, "oracle", "libal_oracle.so")), "o_ksw_extd2", OKsw, False)


def cigar_str(cig):
    return "".join("%d%s" % (int(c) >> 4, "MIDN"[int(c) & 15]) for c in cig) or "*"

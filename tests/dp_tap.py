"""The two device taps of the extension DP for in-process tests: al_dbg_ksw (d_ksw_extd2 / d_ksw_reg, d_ksw_pk with AL_DBG bit 20, on caller-supplied
byte sequences) and al_dbg_ext_dp (the align stage's own kernels by class, on jobs that name a read of an uploaded batch and a reference
position), and the comparison of what they return with ksw_extd2_sse (dp_cases.ref_dp).  Jobs are dp_cases.Job."""
import ctypes as C

import numpy as np

import dp_cases as D

TAP_FIELDS = ("score", "max", "max_q", "max_t", "mqe", "mqe_t", "zdropped", "reach_end")     # al_dbg_ksw: out9[0..7]; out9[8] = n_cigar
COMP = np.array([3, 2, 1, 0, 4], dtype=np.uint8)


def set_options(idx, o):
    m = idx.mo
    m.a, m.b, m.q, m.e, m.q2, m.e2, m.sc_ambi, m.zdrop, m.bw, m.end_bonus = o


def text(codes):
    return bytes(b"ACGTN"[c] for c in codes)


def describe(o, j):
    return "options %s: tlen %d qlen %d flag 0x%x kind %s\n  target %s\n  query  %s" % (tuple(o), len(j.target), len(j.query), j.flag, j.kind, text(j.target).decode(), text(j.query).decode())


def ksw_tap(idx, o, jobs, cap):
    """al_dbg_ksw on jobs under the options o: (out9 [n, 9], cigar words [n, cap]).  The form is chosen by AL_DBG in the environment when the
    context is created (bit 20: two cells per lane)."""
    import airlift_amd as A
    n = len(jobs)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(j.target) + len(j.query) for j in jobs])
    seqs = np.concatenate([x for j in jobs for x in (j.target, j.query)])
    tab = np.zeros((n, 6), dtype=np.int32)
    for i, j in enumerate(jobs):
        tab[i] = (off[i], off[i] + len(j.target), len(j.target), len(j.query), j.flag, 0)
    set_options(idx, o)
    ctx = A.Context(idx)
    set_options(idx, D.SR)
    out = np.full((n, 9), -777, dtype=np.int32); cig = np.zeros((n, cap), dtype=np.uint32)
    rc = A.load().al_dbg_ksw(ctx.h, n, seqs.ctypes.data_as(C.c_void_p), seqs.nbytes, tab.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), cig.ctypes.data_as(C.c_void_p), cap)
    ctx.close()
    assert rc == 0
    return out, cig


def compare_ksw_tap(o, jobs, want, out, cig, what):
    bad = []
    for i, (j, (rf, rcig)) in enumerate(zip(jobs, want)):
        for k, name in enumerate(TAP_FIELDS):
            if int(out[i, k]) != rf[name]:
                bad.append("%s\n  [%s] %s: device %d, reference %d" % (describe(o, j), what, name, out[i, k], rf[name]))
        ng = int(out[i, 8])
        assert 0 <= ng <= cig.shape[1], describe(o, j)
        if tuple(int(c) for c in cig[i, :ng]) != rcig:
            bad.append("%s\n  [%s] CIGAR: device %s, reference %s" % (describe(o, j), what, D.cigar_str(cig[i, :ng]), D.cigar_str(rcig)))
        if len(bad) >= 4:
            break
    assert not bad, "\n".join(bad)


def place(jobs, lmax, seed=11, reads=None):
    """A synthetic reference and batch for jobs: every target lies in the contig behind 8 spacer bases (reversed for a left extension, whose
    target[i] = reference[tpos - i]), every query inside a read of its own.  reads (optional): per job (read length, first read position of
    the query in mapping orientation, strand); otherwise seeded choices as tests/helpers/dp_directed_child.py makes them.
    Returns (reference text, read texts, the al_dbg_ext_dp job table)."""
    rng = np.random.default_rng(seed)
    contig = []; pos = 0; tab = np.zeros((len(jobs), 8), dtype=np.int64); texts = []
    for i, j in enumerate(jobs):
        left = j.flag == D.FLAG_LEFT_EXT
        tl, ql = len(j.target), len(j.query)
        contig += [rng.integers(0, 4, 8, dtype=np.uint8), j.target[::-1] if left else j.target]
        tpos = pos + 8 + (tl - 1 if left else 0)
        pos += 8 + tl
        if reads is not None:
            rl, a, rev = reads[i]
        else:
            rev = (i >> 1) & 1
            rl = lmax if i == 0 else min(lmax, ql + int(rng.integers(0, 40)))        # (the batch's longest read fixes the stage's geometry)
            a = int(rng.integers(0, rl - ql + 1))
        assert 0 <= a and a + ql <= rl <= lmax
        r = rng.integers(0, 4, rl, dtype=np.uint8)                                  # the read in mapping orientation
        r[a:a + ql] = j.query[::-1] if left else j.query
        texts.append(text(COMP[r[::-1]] if rev else r))
        tab[i] = (i, rev, 0 if left else 1, a + ql - 1 if left else a, ql, 0, tpos, tl)
    contig.append(rng.integers(0, 4, 64, dtype=np.uint8))
    return text(np.concatenate(contig)), texts, tab


def ext_dp_tap(o, jobs, lmax, cap, seed=11, reads=None):
    """al_dbg_ext_dp on jobs: ([{field: value}], cigar words [n, cap], the shadow counters).  The environment switches that are read per context
    (AL_DP_EXIT, AL_DP_EXIT_STRIDE, AL_DBG, AL_DBG2) are the caller's."""
    import airlift_amd as A
    n = len(jobs)
    refseq, texts, tab = place(jobs, lmax, seed, reads)
    idx = A.Index(seqs=[refseq], names=[b"chr"])
    set_options(idx, o)
    ctx = A.Context(idx)
    ctx.upload([1] * n, texts, [b"r%d" % i for i in range(n)])
    ctx.run()
    out = np.full((n, 9), -777, dtype=np.int32); cig = np.zeros((n, cap), dtype=np.uint32); shadow = np.zeros(8, dtype=np.uint64)
    rc = A.load().al_dbg_ext_dp(ctx.h, n, tab.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), cig.ctypes.data_as(C.c_void_p), cap, shadow.ctypes.data_as(C.c_void_p))
    ctx.close(); idx.close()
    assert rc == 0
    names = ("max", "max_q", "max_t", "mqe_t", "reach_end", "zdropped", "n_cigar", "class", "lost")
    return [dict(zip(names, (int(x) for x in out[i]))) for i in range(n)], cig, [int(x) for x in shadow]


def compare_ext_dp(o, jobs, want, got, cig, what, zdropped=False):
    """max, max_q, max_t, reach_end, mqe_t when the end is reached, and the CIGAR: what an extension job's caller reads; zdropped as
    well where the caller knows that the early exit cannot fire."""
    bad = []
    for i, (j, (rf, rcig)) in enumerate(zip(jobs, want)):
        g = got[i]
        tag = "%s\n  [%s, job %d, class %d]" % (describe(o, j), what, i, g["class"])
        assert not g["lost"] and 0 <= g["n_cigar"] <= cig.shape[1], tag
        for k in ["max", "max_q", "max_t", "reach_end"] + (["mqe_t"] if rf["reach_end"] else []) + (["zdropped"] if zdropped else []):
            if g[k] != rf[k]:
                bad.append("%s %s: device %d, reference %d" % (tag, k, g[k], rf[k]))
        if tuple(int(c) for c in cig[i, :g["n_cigar"]]) != rcig:
            bad.append("%s CIGAR: device %s, reference %s" % (tag, D.cigar_str(cig[i, :g["n_cigar"]]), D.cigar_str(rcig)))
        if len(bad) >= 4:
            break
    assert not bad, "\n".join(bad)

"""One configuration of tests/test_gpu_dp_directed.py's part two, in a process of its own (AL_DP_PK and its like are read once per process):
the directed cases of tests/dp_cases.py as extension jobs through the align stage's DP kernels (al_dbg_ext_dp) against ksw_extd2_sse.

usage: dp_directed_child.py <option set> <longest read> <full|sparse>      (the environment carries AL_DP_EXIT, AL_DP_PK, AL_DP_PK32, AL_DBG, AL_DBG2)
Prints one JSON line with what was covered; exits 1 with the failing jobs in full on a difference."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import dp_cases as D  # noqa: E402

CLASS_NAMES = {0: "lane16", 1: "lane32", 3: "g1", 4: "g2", 5: "g4", 6: "g8", 8: "g32", 9: "lds"}


def slice_name(cls, tlen):
    """The launch a job of class cls takes: class 7 is three kernels by block count."""
    if cls != 7:
        return CLASS_NAMES[cls]
    b = (tlen + 15) // 16
    return "g12" if b <= 12 else "g16" if b <= 16 else "g22"


def limits(o, lmax):
    """What k_ext_prep can emit for a batch whose longest read has lmax bases (align.c:613-620 and the stage's tiles): (longest target, longest query)."""
    ext = lmax + ((lmax * o.a + o.end_bonus - o.q) // o.e if lmax * o.a + o.end_bonus > o.q else 0)
    tbound = max(2 * lmax + 16, ext + 16)
    tmax = 336 if lmax <= 160 and tbound <= 336 else 512 if lmax <= 256 and tbound <= 512 else 1024 if lmax <= 512 and tbound <= 1024 else 0
    qmax = 160 if tmax == 336 else 256 if tmax == 512 else 512
    assert tmax > 0, "reads of %d bases leave the stage no DP jobs under %s" % (lmax, (o,))
    return min(tmax, tbound), min(qmax, lmax)


def sparse_jobs(max_t, max_q):
    """One or two jobs of each direction per block count: the stage's sort (direction is a key bit below the block count) then leaves wavefronts
    that hold both directions."""
    out = []
    for b in range(1, (max_t + 15) // 16 + 1):
        for k, flag in enumerate((D.FLAG_LEFT_EXT, D.FLAG_RIGHT_EXT, D.FLAG_LEFT_EXT)[:2 + b % 2]):
            T = min(max_t, 16 * b - (b * 5 + k * 3) % 16)
            Q = max(1, min(max_q, (T + 1) // 2 + 7 * k if b % 3 else T))
            kind = D.KIND_NAMES[(b * 3 + k) % len(D.KIND_NAMES)]
            t, q = D.make_pair(T, Q, kind)
            out.append(D.Job(t, q, flag, kind))
    return out


def main():
    optname, lmax, mode = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    import airlift_amd as A
    o = D.OPTION_SETS[optname]
    max_t, max_q = limits(o, lmax)
    jobs = D.cases(D.FLAGS_PRODUCTION, max_t, max_q) if mode == "full" else sparse_jobs(max_t, max_q)
    n = len(jobs)
    ref = D.ref_dp()
    want = [ref(o, j) for j in jobs]
    rng = np.random.default_rng(11)
    # the synthetic reference (targets, spaced) and the batch (a read per job, the query somewhere inside it)
    contig = []; pos = 0; tab = np.zeros((n, 8), dtype=np.int64); reads = []
    comp = np.array([3, 2, 1, 0, 4], dtype=np.uint8)
    for i, j in enumerate(jobs):
        left = j.flag == D.FLAG_LEFT_EXT; rev = (i >> 1) & 1
        tl, ql = len(j.target), len(j.query)
        sp = rng.integers(0, 4, 8, dtype=np.uint8)
        contig += [sp, j.target[::-1] if left else j.target]
        tpos = pos + 8 + (tl - 1 if left else 0)                            # left: target[i] = reference[tpos - i]
        pos += 8 + tl
        rl = min(lmax, ql + int(rng.integers(0, 40)))
        if i == 0:
            rl = lmax                                                       # the batch's longest read fixes the stage's geometry
        a = int(rng.integers(0, rl - ql + 1))
        r = rng.integers(0, 4, rl, dtype=np.uint8)                          # the read in mapping orientation
        r[a:a + ql] = j.query[::-1] if left else j.query
        qoff = a + ql - 1 if left else a
        reads.append(bytes(b"ACGTN"[c] for c in (comp[r[::-1]] if rev else r)))
        tab[i] = (i, rev, 0 if left else 1, qoff, ql, 0, tpos, tl)
    contig.append(rng.integers(0, 4, 64, dtype=np.uint8))
    refseq = bytes(b"ACGTN"[c] for c in np.concatenate(contig))
    idx = A.Index(seqs=[refseq], names=[b"chr"])
    m = idx.mo
    m.a, m.b, m.q, m.e, m.q2, m.e2, m.sc_ambi, m.zdrop, m.bw, m.end_bonus = o
    ctx = A.Context(idx)
    ctx.upload([1] * n, reads, [b"r%d" % i for i in range(n)])
    ctx.run()
    cap = max(len(c) for _, c in want) + 1
    out = np.full((n, 9), -777, dtype=np.int32); cig = np.zeros((n, cap), dtype=np.uint32); shadow = np.zeros(8, dtype=np.uint64)
    rc = A.load().al_dbg_ext_dp(ctx.h, n, tab.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), cig.ctypes.data_as(C.c_void_p), cap, shadow.ctypes.data_as(C.c_void_p))
    dp_jobs = list(ctx.stat().dp_jobs)
    ctx.close(); idx.close()
    if rc != 0:
        print("al_dbg_ext_dp returned %d" % rc); sys.exit(1)
    env = os.environ
    dbg2 = int(env.get("AL_DBG2", "0")); shadow_on = bool(dbg2 & 32)
    pk = env.get("AL_DP_PK", "1") != "0" and D.PK_OK[optname]
    pk32 = pk and env.get("AL_DP_PK32", "1") != "0"
    exit_on = env.get("AL_DP_EXIT", "1") != "0" and not shadow_on and o.q + o.e <= o.q2 + o.e2
    bad = []; compared = 0; cover = {}; zd_compared = 0
    for i, (j, (rf, rcig)) in enumerate(zip(jobs, want)):
        compared += 1
        g = dict(zip(("max", "max_q", "max_t", "mqe_t", "reach_end", "zdropped", "n_cigar", "class", "lost"), (int(x) for x in out[i])))
        where = slice_name(g["class"], len(j.target)) if g["class"] in CLASS_NAMES or g["class"] == 7 else "class %d" % g["class"]
        tag = "%s\n  [%s, read %d rev %d kind %d]" % (D.describe(optname, j), where, i, tab[i, 1], tab[i, 2])
        if g["lost"] or not 0 <= g["n_cigar"] <= cap:
            bad.append("%s CIGAR of %d words not returned whole (asked for %d)" % (tag, g["n_cigar"], cap)); continue
        names = ["max", "max_q", "max_t", "reach_end"] + (["mqe_t"] if rf["reach_end"] else [])
        # under the early exit only the fields above are kept: zdropped where the exit is not compiled in (below 12 target blocks, one-cell form) or is off
        exit_here = exit_on and ((g["class"] == 7 and pk) or (g["class"] == 8 and pk32))
        if not exit_here:
            names.append("zdropped"); zd_compared += 1
        for k in names:
            if g[k] != rf[k]:
                bad.append("%s %s: device %d, reference %d" % (tag, k, g[k], rf[k]))
        if tuple(int(c) for c in cig[i, :g["n_cigar"]]) != rcig:
            bad.append("%s CIGAR: device %s, reference %s" % (tag, D.cigar_str(cig[i, :g["n_cigar"]]), D.cigar_str(rcig)))
        c = cover.setdefault(where, {"left": 0, "right": 0, "rev0": 0, "rev1": 0})
        c["left" if tab[i, 2] == 0 else "right"] += 1; c["rev%d" % tab[i, 1]] += 1
        if len(bad) >= 6:
            break
    if bad:
        print("\n".join(bad)); sys.exit(1)
    # jobs per (block count, direction): how full the sorted list's runs of one direction are
    runs = {}
    for i, j in enumerate(jobs):
        runs.setdefault(((len(j.target) + 15) // 16, int(tab[i, 2])), 0); runs[((len(j.target) + 15) // 16, int(tab[i, 2]))] += 1
    print(json.dumps({"generated": n, "compared": compared, "zdropped_compared": zd_compared, "cover": cover, "dp_jobs": dp_jobs, "shadow": [int(x) for x in shadow],
                      "run_min": min(runs.values()), "run_max": max(runs.values()), "limits": [max_t, max_q]}))


if __name__ == "__main__":
    main()

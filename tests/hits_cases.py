"""Directed chain sets for the stage between chaining and extension -- a fragment's chains to its per-mate hits -- shared by
tests/test_hits_oracle_cpu.py and tests/test_gpu_hits_directed.py, and the ctypes view of what they are compared with: the reference's mm_gen_regs,
mm_set_parent, mm_select_sub(_multi), mm_seg_gen, mm_squeeze_a and mm_set_mapq behind oracle/hitref_shim.c (oracle/_ref/libhitref.so, built by
oracle/Makefile), and the oracle's o_frag_hits.

A fragment is (qlens, rep_len, u, anchors, label): the mates' read lengths, its rep_len, its chains as u[] (score << 32 | anchors) and their anchors
packed chain after chain as an (n, 2) uint64 array
    x = rev << 63 | rid << 32 | pos          y = seg << 48 | span << 32 | qpos
with qpos in the fragment's concatenated coordinates (the reverse strand: of the reversed fragment, mate 1 first).  The chains are the caller's own:
scores and counts are free of what chaining would give.  Everything is deterministic: every family's generator is seeded by its name, and fragment i
of a list is mapped under the name f<i>, which fixes its hash.  What the families aim at follows from what the kernels branch on (k_regs_select's
classes and bail-outs, k_regs_heavy's tiles, k_regs and its one-chain path, k_map_only(_wave)); tests/test_hits_oracle_cpu.py proves on the
reference alone that the list reaches them."""
import ctypes as C
import os
import subprocess
import zlib
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

Opt = namedtuple("Opt", "mask_level pri_ratio best_n k max_gap max_gap_ref max_frag_len min_chain_score a b")
SR = Opt(0.5, 0.5, 20, 21, 100, -1, 800, 25, 2, 8)             # -x sr (options.c)
OPTION_SETS = {
    "sr": SR,
    "best_n1": SR._replace(best_n=1),
    "best_n150": SR._replace(best_n=150),
    "pri_ratio0": SR._replace(pri_ratio=0.0),                  # mm_select_sub(_multi) keep everything
    "mask03": SR._replace(mask_level=0.3),
    "mask09": SR._replace(mask_level=0.9),
    "k15": SR._replace(k=15),                                  # min_diff = 2 k
    "k28": SR._replace(k=28),
    "max_gap_ref300": SR._replace(max_gap_ref=300),
    "max_frag_len1200": SR._replace(max_frag_len=1200),
}
CHAIN_COUNTS = (0, 1, 2, 4, 5, 63, 64, 65, 256, 257, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16500)
CLASS_EDGES = (5, 65, 257, 1025, 2049, 4097, 8193)            # k_regs_select: <0> 5-64, <256>, <1024>, <2048>, <4096>, <8192,1>, <-1> above
HEAVY_TILES = ((12, 256), (24, 512), (48, 768), (72, 1024), (200, 2048))   # k_regs_heavy: (kept hits, anchors)
HEAVY_KEPT = (8, 9, 12, 13, 24, 25, 48, 49, 72, 73, 200, 201)
HEAVY_ANCHORS = (256, 257, 512, 513, 768, 769, 1024, 1025, 2048, 2049)
PMAX, KCAP, MO_LIGHT, LOGTAB_N = 64, 96, 4, 16384             # the kernels' constants of these names (al_kernels_align.hip, al_device.h)
SERIAL_MAX_CHAINS = 2100                                       # the all-serial configuration takes the fragments of at most this many chains
PE, SE = (150, 150), (150,)
SEED = 11                                                      # mm_mapopt_t::seed

Frag = namedtuple("Frag", "qlens rep_len u anchors label")
# a chain before it is packed: score and its anchors as rows of (rev, rid, pos, seg, qpos)
Chain = namedtuple("Chain", "score pts")


def max_gap_ref(o, qlens):
    """max_chain_gap_ref of a fragment (map.c:344-349), what mm_select_sub_multi's max_dist is made of."""
    qs = sum(qlens)
    if o.max_gap_ref > 0:
        return o.max_gap_ref
    if o.max_frag_len > 0:
        return max(o.max_frag_len - qs, o.max_gap)
    return o.max_gap


def _rng(name):
    return np.random.default_rng([20250907, zlib.crc32(name.encode())])


def _seg_of(qlens, rev, y, span):
    """The mate an anchor at concatenated query position y lies in, or None where its k-mer would straddle the two mates."""
    if len(qlens) == 1:
        return 0
    first = qlens[1] if rev else qlens[0]                       # (the reversed fragment starts with mate 1)
    if y < first:
        return 1 if rev else 0
    if y + 1 - span < first:
        return None
    return 0 if rev else 1


def hit(o, qlens, score, qs, qe, pos, cnt=2, rev=0, rid=0, dy_last=0):
    """A chain of (up to) cnt anchors on one diagonal whose fragment-level hit covers the query interval [qs, qe) (hit.c:23-38) and starts at reference
    position pos + 1 - k.  dy_last moves the last anchor (two chains with equal first anchors and different ends)."""
    span = o.k; qsum = sum(qlens)
    assert 0 <= qs and qe <= qsum and qe - qs >= span, (qs, qe, qsum)
    y0, y1 = (qs + span - 1, qe - 1) if not rev else (qsum - qe + span - 1, qsum - qs - 1)
    ys = sorted(set(int(v) for v in np.linspace(y0, y1, max(cnt, 1)).round())) if cnt > 1 and y1 > y0 else [y0]
    pts = []
    for y in ys:
        s = _seg_of(qlens, rev, y, span)
        if s is not None:
            pts.append((rev, rid, pos + (y - y0), s, y))
    assert pts, (qlens, qs, qe)
    if dy_last and len(pts) > 1:
        r, d, p, s, y = pts[-1]
        if _seg_of(qlens, rev, y + dy_last, span) == s and y + dy_last < qsum and y + dy_last > pts[-2][4]:
            pts[-1] = (r, d, p + dy_last, s, y + dy_last)
    return Chain(score, pts)


def dense_chain(o, qlens, score, cnt, pos):
    """A chain of exactly cnt anchors a base apart, from the first bases of the fragment on (over the mate boundary where one mate has too few)."""
    ys = [y for y in range(o.k + 1, sum(qlens)) if _seg_of(qlens, 0, y, o.k) is not None][:cnt]
    assert len(ys) == cnt, (qlens, cnt)
    return Chain(score, [(0, 0, pos + y - ys[0], _seg_of(qlens, 0, y, o.k), y) for y in ys])


def frag(o, qlens, chains, label, rep_len=0):
    span = o.k
    u = np.array([(c.score << 32) | len(c.pts) for c in chains], dtype=np.uint64)
    rows = [p for c in chains for p in c.pts]
    a = np.array(rows, dtype=np.int64).reshape(-1, 5).astype(np.uint64)
    x = a[:, 0] << np.uint64(63) | a[:, 1] << np.uint64(32) | a[:, 2]
    y = a[:, 3] << np.uint64(48) | np.uint64(span) << np.uint64(32) | a[:, 4]
    assert len(a) == 0 or (int(a[:, 2].max()) < 1 << 31 and int(a[:, 4].max()) < sum(qlens)), label
    assert all(0 < c.score < 1 << 31 and c.pts for c in chains), label
    return Frag(tuple(qlens), rep_len, u, np.ascontiguousarray(np.stack([x, y], axis=1)), label)


def _regions(qlens, width, gap=4):
    """Disjoint query intervals of `width` bases that tile the fragment, none across the mate boundary."""
    out, base = [], 0
    for L in qlens:
        out += [(base + s, base + s + width) for s in range(0, L - width + 1, width + gap)]
        base += L
    return out


# ---- the families --------------------------------------------------------------------------------------------------------------------
def _repeat_like(o, g, qlens, n, label, n_pri=3, two=None, score_hi=None):
    """n chains as a read inside a repeat has them: a few query regions, every chain over one of them at a reference position of its own (both
    strands, two contigs, near the best chain and far from it), scores spread so that some secondaries pass every threshold and some none.
    two: how many chains have two anchors (the others one)."""
    qsum = sum(qlens); k = o.k
    w = min(max(k + 9, qsum // (n_pri + 1)), 120)
    regs = _regions(qlens, w)
    regs = [regs[int(i)] for i in np.linspace(0, len(regs) - 1, min(n_pri, len(regs))).round()]
    hi = score_hi or 2 * w
    chains = []
    for i in range(n):
        qs, qe = regs[i % len(regs)]
        if i >= len(regs) and g.random() < 0.3:                   # a part of the region, or across two of them
            d = int(g.integers(0, w - k)); qs, qe = (qs + d, qe) if g.random() < 0.5 else (qs, qe - d)
        score = hi - i % len(regs) if i < len(regs) else int(g.integers(max(hi // 8, 1), hi - len(regs)))
        near = g.random() < 0.5
        pos = 50000 + (int(g.integers(0, 600)) if near else 3000 + 997 * i % 2000000)
        cnt = 2 if two is None or i < two else 1
        chains.append(hit(o, qlens, score, qs, qe, pos, cnt=cnt, rev=int(g.random() < 0.3), rid=int(g.random() < 0.15)))
    order = g.permutation(n)                                     # (the chain stage's order is by position, not by score)
    return frag(o, qlens, [chains[i] for i in order], label, rep_len=int(g.integers(0, 3)) * 7)


def counts(o):
    out = []
    g = _rng("counts")
    for n in CHAIN_COUNTS:
        for qlens in (PE, SE):
            if n == 16500 and qlens == SE:
                continue                                         # (the single-end fragment of that size is mapq()'s)
            two = None if n < 8192 else 9000 - n if n < 16500 else None
            out.append(_repeat_like(o, g, qlens, n, "counts %d chains %s" % (n, qlens), two=two))
    for n in (6, 30, 100, 300, 700):                              # more of the small classes, a primary more or less
        for j, qlens in enumerate((PE, SE, (300,), (250, 100))):
            out.append(_repeat_like(o, g, qlens, n, "counts %d chains %s #%d" % (n, qlens, j), n_pri=1 + (n + j) % 5))
    return out


READ_LENGTHS = ((300,), (2048,), (2049,), (1024, 1024), (1025, 1024), (32766, 32767), (32767, 32767))
# Fragments of 65535 and 65536 bases: the latter's query coordinates do not fit the 16 bits of the selection kernels' tables (their bail-out 0xfffffff3).  No
# batch holds one: al_batch_upload refuses a read of 32768 bases, so a pair has at most 65534.  The oracle is compared with the reference on them;
# the kernels get the longest pairs there are, above.
HOST_ONLY_READ_LENGTHS = ((32767, 32768), (32768, 32768))
MAX_READ_LEN = 32767


def read_lengths(o, lengths=READ_LENGTHS):
    """The coverage bitmap holds 2048 bases, above it an interval sweep; the query coordinates of the longest pair still fit 16 bits."""
    out = []
    g = _rng("lengths")
    for qlens in lengths:
        qsum = sum(qlens)
        for n in (3, 40, 100, 300):
            out.append(_repeat_like(o, g, qlens, n, "lengths %s %d chains" % (qlens, n), n_pri=4))
        # chains up to the last base, over it a chain that two primaries cover in part
        w = 60
        ch = [hit(o, qlens, 500, qsum - w, qsum, 70000), hit(o, qlens, 480, qsum - 3 * w, qsum - 2 * w, 71000), hit(o, qlens, 300, qsum - 3 * w + 20, qsum - 10, 90000, cnt=3),
              hit(o, qlens, 290, qsum - w - 5, qsum, 91000, rev=1), hit(o, qlens, 280, 0, w, 92000), hit(o, qlens, 270, 0, w + 30, 93000, rev=1), hit(o, qlens, 200, qsum - w, qsum, 94000, rid=1)]
        out.append(frag(o, qlens, ch, "lengths %s last bases" % (qlens,)))
    return out


def primaries(o):
    """1 ... 65 primaries from short chains tiling the query; overlaps around mask_level, on it, and chains over two or three primaries."""
    out = []
    g = _rng("primaries")
    k = o.k; w = k + 5
    for qlens in ((2400,), (1200, 1200)):
        regs = _regions(qlens, w, gap=3)
        assert len(regs) >= 66
        for P in (1, 2, 63, 64, 65):
            pick = [regs[int(i)] for i in np.linspace(0, len(regs) - 1, P).round()] if P > 1 else [regs[3]]
            ch = [hit(o, qlens, 900 - i, qs, qe, 20000 + 500 * i) for i, (qs, qe) in enumerate(pick)]
            for j in range(12):                                   # secondaries of some of them, above and below the thresholds
                qs, qe = pick[(j * 7) % P]
                ch.append(hit(o, qlens, (800, 460, 440, 300)[j % 4] - j, qs, qe, 900000 + 700 * j, rev=j & 1))
            out.append(frag(o, qlens, [ch[i] for i in g.permutation(len(ch))], "primaries %d %s" % (P, qlens)))
    # a primary [100, 140) and a chain of L2 bases that overlaps it by ol: (float)ol / min - (float)uncov / max against mask_level, every ol
    for qlens in (PE, SE):
        if sum(qlens) < 140 + 60:
            continue
        for L2 in (40, 60):
            for ol in range(0, 41):
                if L2 < max(k, 1) or 140 - ol + L2 > qlens[0] or 40 < k:
                    continue
                ch = [hit(o, qlens, 300, 100, 140, 30000), hit(o, qlens, 200, 140 - ol, 140 - ol + L2, 60000)]
                out.append(frag(o, qlens, ch, "primaries overlap %d of a chain of %d %s" % (ol, L2, qlens)))
    # three primaries with gaps between them, a chain over two or three of them: uncov_len counts the gaps and the ends
    for qlens in ((300,), (2049,), (150, 150)):
        w3 = max(40, k + 4)
        if qlens == (150, 150):
            pr = [(0, w3), (w3 + 20, 2 * w3 + 20), (150 + 10, 150 + 10 + w3)]
        else:
            pr = [(0, w3), (w3 + 20, 2 * w3 + 20), (2 * w3 + 40, 3 * w3 + 40)]
        for d in (0, 5, 15, w3 - 1):
            for e in (0, 7, 19):
                for last in (1, 2):
                    qs, qe = pr[0][0] + d, pr[last][1] - e + (10 if last == 2 and qlens != (150, 150) else 0)
                    if qe - qs < k or qe > sum(qlens):
                        continue
                    ch = [hit(o, qlens, 500 - i, a, b, 40000 + 3000 * i) for i, (a, b) in enumerate(pr)]
                    ch.append(hit(o, qlens, 260, qs, qe, 80000, cnt=4))
                    ch.append(hit(o, qlens, 255, qs + 1, qe, 85000, cnt=3, rev=1))
                    out.append(frag(o, qlens, ch, "primaries chain over %d of three, in by %d and %d %s" % (last + 1, d, e, qlens)))
    return out


def selection(o):
    """mm_select_sub / mm_select_sub_multi: scores around parent * pri_ratio, * 0.2f, * 0.7f and parent - 2 k; identical hits; mates near and far,
    on the other strand, on another contig, hits across the mate boundary; best_n - 1, best_n, best_n + 1 qualifiers."""
    out = []
    k = o.k
    for qlens in (PE, SE):
        mgr = max_gap_ref(o, qlens); md = sum(qlens) + mgr
        paired = len(qlens) == 2
        w = 60
        ctx = [("same place", dict(pos=50100)), ("other strand", dict(pos=50100, rev=1)), ("other contig", dict(pos=50100, rid=1))]
        for e in (-1, 0, 1):                                      # q->re - p->rs and p->re - q->rs around max_dist (hits of w bases: re - rs = w)
            ctx.append(("right of it, re - rs = max_dist%+d" % e, dict(pos=50000 + md + e - w)))
            ctx.append(("left of it, re - rs = max_dist%+d" % e, dict(pos=50000 - (md + e - w))))
        for P in (200, 333, 101, 97, 1000):
            thr = sorted({int(P * r) + d for r in (o.pri_ratio, 0.2, 0.7) for d in (-1, 0, 1)} | {P - 2 * k + d for d in (-1, 0, 1)})
            thr = [t for t in thr if 0 < t <= P]
            for name, kw in ctx:
                spans = ((40, 40 + w, "mate 0"),) + (((120, 120 + w, "both mates"),) if paired else ())
                for pqs, pqe, pname in spans:
                    for cqs, cqe, cname in spans:
                        if P not in (200, 97) and (pname, cname) != ("mate 0", "mate 0"):
                            continue
                        ch = [hit(o, qlens, P, pqs, pqe, 50000, cnt=4)]
                        ch += [hit(o, qlens, t, cqs, cqe, kw["pos"] + 3 * j, rev=kw.get("rev", 0), rid=kw.get("rid", 0), cnt=2 + j % 3) for j, t in enumerate(thr)]
                        out.append(frag(o, qlens, ch[::-1], "selection parent %d (%s), secondaries (%s) %s %s" % (P, pname, cname, name, qlens)))
        # hits identical to the parent (coordinates equal, another score), and one that differs by a base
        ch = [hit(o, qlens, 200, 40, 100, 50000, cnt=3), hit(o, qlens, 190, 40, 100, 50000, cnt=2), hit(o, qlens, 180, 40, 100, 50000, cnt=3), hit(o, qlens, 170, 40, 101, 50000, cnt=3),
              hit(o, qlens, 160, 40, 100, 50000, cnt=3, rid=1), hit(o, qlens, 150, 40, 100, 50000, cnt=3, rev=1)]
        out.append(frag(o, qlens, ch, "selection hits identical to the parent %s" % (qlens,)))
        # a parent and best_n + d secondaries that qualify, then some that do not, a second primary with its own
        for d in (-1, 0, 1):
            nq = max(o.best_n + d, 0)
            ch = [hit(o, qlens, 1000, 10, 70, 50000, cnt=3)] + [hit(o, qlens, 990 - j, 10, 70, 60000 + 300 * j) for j in range(nq)]
            ch += [hit(o, qlens, 100 - j, 10, 70, 40000 - 300 * j) for j in range(3)]
            ch += [hit(o, qlens, 400, 80, 140, 70000)] + [hit(o, qlens, 399 - j, 80, 140, 200000 + 300 * j, rid=1) for j in range(2)]
            out.append(frag(o, qlens, ch, "selection best_n%+d qualifiers %s" % (d, qlens)))
    return out


def compaction(o):
    """The reference's selection moves the kept hits to the front of the same array and looks a secondary's parent up at its OLD index: once more hits
    have been kept than that index, the slot holds another hit.  Parent B at old index p = (primaries before it) + (dropped secondaries before it),
    then kept hits, then secondaries of B around the thresholds of B's score and of the scores now found at slot p."""
    out = []
    k = o.k; w = k + 5
    shapes = [(1, 2, 4, 2), (2, 8, 4, 10), (3, 17, 8, 14), (5, 1, 2, 6), (2, 40, 30, 15), (30, 30, 26, 10), (35, 35, 27, 12), (20, 43, 40, 10), (10, 60, 52, 20),
              (40, 55, 45, 20), (30, 66, 50, 20), (30, 67, 50, 20), (50, 47, 60, 20), (50, 50, 60, 0),
              (30, 65, 10, 60), (30, 66, 10, 60), (30, 67, 10, 60), (20, 110, 20, 95), (60, 36, 3, 40), (2, 93, 50, 50), (2, 94, 50, 50), (2, 95, 50, 50)]
    for n_pb, n_drop, n_bp, n_bs in shapes:
        for qlens in ((4100,), (2048,), (2050, 2050)):
            regs = _regions(qlens, w, gap=3)
            if n_pb + 1 + n_bp > len(regs):
                continue
            p = n_pb + n_drop
            sec = dict(rid=1)                                     # (another contig: mm_select_sub_multi takes the pri_ratio branch as mm_select_sub does)
            ch = [hit(o, qlens, 5000 if i == 0 else 4000 - i, *regs[i], 10000 + 400 * i) for i in range(n_pb)]
            ch += [hit(o, qlens, 2400 - j, *regs[0], 500000 + 400 * j, **sec) for j in range(n_drop)]
            ch.append(hit(o, qlens, 2000, *regs[n_pb], 30000))                                     # B
            between = [(1990 - 2 * j, regs[n_pb + 1 + j], {}) for j in range(n_bp)] + [(1989 - 2 * j, regs[n_pb], sec) for j in range(n_bs)]
            ch += [hit(o, qlens, s, *r, 900000 + 400 * j, **kw) for j, (s, r, kw) in enumerate(between)]
            tested = [1001, 1000, 999, 996, 995, 994, 990, 985, 980, 975, 970, 960, 950, 940, 930, 920]
            ch += [hit(o, qlens, s, *regs[n_pb], 1500000 + 400 * j, **sec) for j, s in enumerate(tested)]
            out.append(frag(o, qlens, ch[::-1], "compaction parent at %d (%d primaries, %d dropped before it), %d + %d kept after %s" % (p, n_pb, n_drop, n_bp, n_bs, qlens)))
    return out


def ties(o):
    """Equal sort keys from duplicated chains (same u, same first anchor; the ends differ, so that their order shows): the reference's radix sort is
    an insertion sort up to 64 chains and not stable above."""
    out = []
    g = _rng("ties")
    for n, dup in ((5, 2), (6, 3), (40, 2), (40, 3), (64, 2), (64, 3), (65, 2), (65, 3), (300, 2), (300, 3), (5000, 2), (5000, 3), (300, 70), (1200, 100), (200, 65), (64, 30)):
        for qlens in (PE, SE):
            base = _repeat_like(o, g, qlens, n - dup + 1, "x", n_pri=2)
            # duplicate one chain of at least two anchors dup - 1 times, its last anchor moved
            nu = (base.u & np.uint64(0xffffffff)).astype(np.int64); off = np.concatenate([[0], np.cumsum(nu)])
            for which, tag in ((int(np.argmax(base.u >> np.uint64(32))), "the best chain"), (int(np.argsort(base.u >> np.uint64(32))[len(nu) // 2]), "a middle chain")):
                if nu[which] < 2:
                    continue
                us, an = list(base.u), [base.anchors[off[i]:off[i + 1]] for i in range(len(nu))]
                for j in range(1, dup):
                    a = an[which].copy()
                    a[-1, 0] += np.uint64(j % 7); a[-1, 1] += np.uint64(0)       # (the reference position of the last anchor: re differs, the key does not)
                    at = int(g.integers(0, len(us) + 1))
                    us.insert(at, base.u[which]); an.insert(at, a)
                out.append(Frag(qlens, 0, np.array(us, dtype=np.uint64), np.ascontiguousarray(np.concatenate(an)), "ties %d chains, %d copies of %s %s" % (n, dup, tag, qlens)))
    return out


def big_scores(o):
    """A score of 2^16 or more: the 48-bit sort keys of k_regs_select do not hold it.  (Reads long enough for the logf table of a map-only run.)"""
    out = []
    g = _rng("big")
    for qlens in ((20000, 20000), (32767,)):
        for n in (300, 3000):
            for top in (65536, 70000):
                out.append(_repeat_like(o, g, qlens, n, "big score %d among %d chains %s" % (top, n, qlens), n_pri=3, score_hi=top))
    return out


def heavy(o):
    """k_regs_heavy's tiles: (kept hits, their anchors) up to (12, 256), (24, 512), (48, 768), (72, 1024), (200, 2048); what exceeds them is k_regs's."""
    out = []
    k = o.k; w = k + 5
    for kept in HEAVY_KEPT:                                       # primaries tiling the query and min(best_n, ...) secondaries, every one kept
        for qlens in ((4100,), (2050, 2050)):
            regs = _regions(qlens, w, gap=3)
            n_sec = min(o.best_n, max(kept - 3, 0), kept * 2 // 3) if o.pri_ratio > 0 else kept * 2 // 3
            n_pri = kept - n_sec
            if n_pri > len(regs):
                continue
            ch = [hit(o, qlens, 3000 - i, *regs[i], 10000 + 400 * i) for i in range(n_pri)]
            ch += [hit(o, qlens, 2900 - j, *regs[j % n_pri], 700000 + 400 * j, rev=j & 1) for j in range(n_sec)]
            if o.pri_ratio > 0:
                ch += [hit(o, qlens, 100 + j, *regs[j % n_pri], 1700000 + 400 * j) for j in range(5)]    # dropped
            out.append(frag(o, qlens, ch[::-1], "heavy %d kept hits (%d primaries) %s" % (kept, n_pri, qlens)))
    for tot in HEAVY_ANCHORS:                                     # ten kept hits whose anchors add up to tot: the anchor total alone picks the tile
        for qlens in ((300,), (150, 150)):
            per = [tot // 10 + (1 if i < tot % 10 else 0) for i in range(10)]
            ch = [dense_chain(o, qlens, 2000 - i, c, 10000 + 3000 * i) for i, c in enumerate(per)]
            got = sum(len(c.pts) for c in ch)
            assert got == tot
            ch += [hit(o, qlens, 50 + j, 2, 2 + k + 40, 900000 + 3000 * j) for j in range(4)]
            out.append(frag(o, qlens, ch, "heavy ten kept hits of %d anchors (%d) %s" % (tot, got, qlens)))
    return out


def seg_gen(o):
    """mm_seg_gen: chains in mate 0, in mate 1, in both, on both strands; a mate left without chains; per-mate duplicates that tie."""
    out = []
    k = o.k
    for qlens in (PE, (250, 100)):
        q0, qsum = qlens[0], sum(qlens)
        for rev in (0, 1):
            q1 = qlens[1] if rev else q0                           # (the mate the chain's coordinates start in: the reversed fragment starts with mate 1)
            A = dict(m0=(10, 10 + k + 40), m1=(q1 + 5, q1 + 5 + k + 40), both=(q1 - k - 30, q1 + k + 30))
            if rev:
                A["m0"], A["m1"] = A["m1"], A["m0"]
            for combo in (("m0",), ("m1",), ("both",), ("m0", "m1"), ("m0", "both"), ("m1", "both"), ("m0", "m1", "both"), ("m0", "m0"), ("m1", "m1"), ("both", "both", "both")):
                ch = []
                for j, nm in enumerate(combo):
                    qs, qe = A[nm]
                    if rev:
                        qs, qe = qsum - qe, qsum - qs
                    ch.append(hit(o, qlens, 300 - 40 * j, qs, qe, 50000 + 5000 * j, cnt=6, rev=rev))
                out.append(frag(o, qlens, ch, "seg_gen %s %s %s" % ("+".join(combo), "reverse" if rev else "forward", qlens)))
        # two chains with different anchors in mate 0 and the same anchors in mate 1, equal scores: their mate-1 hits have equal keys
        for rev in (0, 1):
            for copies in (2, 3):
                ch = []
                for j in range(copies):
                    m1 = hit(o, qlens, 200, q0 + 5, q0 + 5 + k + 30, 70000 if rev else 80000, cnt=3, rev=rev)
                    m0 = hit(o, qlens, 200, 10 + 3 * j, 10 + k + 30, 80000 + 100 * j if rev else 70000 - 100 * j, cnt=3, rev=rev)
                    pts = (m1.pts + m0.pts) if rev else (m0.pts + m1.pts)
                    ch.append(Chain(200, pts))
                ch.append(hit(o, qlens, 150, q0 + 5, q0 + 5 + k + 30, 300000, cnt=2, rev=rev))
                out.append(frag(o, qlens, ch, "seg_gen %d chains tie in mate 1 %s %s" % (copies, "reverse" if rev else "forward", qlens)))
    return out


def one_chain(o):
    """One chain of a pair (k_regs's fast path): 1, 2 and 40 anchors, every split between the mates, both strands."""
    out = []
    k = o.k
    qlens = PE
    for rev in (0, 1):
        for cnt in (1, 2, 40):
            for c1 in range(cnt + 1):
                first, second = (1, 0) if rev else (0, 1)           # (the reversed fragment starts with mate 1)
                n_first = c1 if rev else cnt - c1
                pts = []
                for i in range(cnt):
                    s = first if i < n_first else second
                    y = (k - 1 + 2 * i) if i < n_first else qlens[first] + k - 1 + 2 * (i - n_first)
                    pts.append((rev, 0, 40000 + 2 * i + (0 if i < n_first else 300), s, y))
                out.append(frag(o, qlens, [Chain(60 + cnt, pts)], "one chain of %d anchors, %d in mate 1, %s" % (cnt, c1, "reverse" if rev else "forward"), rep_len=(0, 10)[c1 & 1]))
    return out


def mapq(o):
    """mm_set_mapq without r->p (map-only runs): score, cnt, subsc around min_chain_score, n_sub, rep_len; mates of 4, 5, 64, 65 and 130 hits; a
    primary with n_sub + 1 above the smallest log table."""
    out = []
    k = o.k; mcs = o.min_chain_score
    qlens = (300,)
    scores = list(range(1, 131)) + list(range(135, 401, 5))
    for i, s in enumerate(scores):                                # a primary of score s with n_sub secondaries of score sub (none where sub is 0)
        cnt = 1 + i % 12
        sub = (0, mcs - 1, mcs, mcs + 1, s // 2, s)[i % 6]
        n_sub = (0, 1, 2, 5, 17, 60, 150, 300)[i % 8] if sub else 0
        if sub > s:
            sub = s
        ch = [hit(o, qlens, s, 10, 10 + k + 60, 50000, cnt=cnt)]
        ch += [hit(o, qlens, max(sub - (j > 0), 1), 10, 10 + k + 60, 60000 + 300 * j, cnt=cnt + (j % 3 == 0)) for j in range(n_sub if sub > 0 else 0)]
        out.append(frag(o, qlens, ch, "mapq score %d cnt %d subsc %d n_sub %d" % (s, cnt, sub, n_sub), rep_len=(0, 10, 5000)[i % 3]))
    for s in (101, 150, 250, 400):                                # score above 100 with every cnt and rep_len
        for cnt in range(1, 13):
            ch = [hit(o, qlens, s, 10, 10 + k + 60, 50000, cnt=cnt), hit(o, qlens, 30 + cnt, 10, 10 + k + 60, 70000, cnt=1 + cnt % 4)]
            out.append(frag(o, qlens, ch, "mapq high score %d cnt %d" % (s, cnt), rep_len=(0, 10, 5000)[cnt % 3]))
    for v in range(60, 200):                                      # one primary of score 200 and one secondary of every score: subsc / score0 swept, n_sub 0 and 1
        ch = [hit(o, qlens, 200, 10, 10 + k + 60, 50000, cnt=12), hit(o, qlens, v, 10, 10 + k + 60, 70000, cnt=11 + (v & 1) * 2)]
        out.append(frag(o, qlens, ch, "mapq score 200 subsc %d" % v))
    for v in range(100, 300):
        ch = [hit(o, qlens, 300, 10, 10 + k + 60, 50000, cnt=12), hit(o, qlens, v, 10, 10 + k + 60, 70000, cnt=11 + (v % 3 == 0) * 2)]
        out.append(frag(o, qlens, ch, "mapq score 300 subsc %d" % v))
    w = k + 5
    for H in (4, 5, 64, 65, 130):                                 # mates of H hits: primaries tiling one mate, up to best_n secondaries; the other mate of a pair has none
        for qlens in ((4100,), (4100, 200)):
            regs = [r for r in _regions(qlens, w, gap=3) if r[1] <= 4100]
            n_sec = min(o.best_n, H // 3) if o.pri_ratio > 0 else H // 3
            n_pri = min(H - n_sec, len(regs))
            ch = [hit(o, qlens, 90 + i % 40, *regs[i], 10000 + 400 * i, cnt=2 + i % 4) for i in range(n_pri)]
            ch += [hit(o, qlens, 80 - j % 9, *regs[j % n_pri], 700000 + 400 * j, cnt=3, rev=j & 1) for j in range(n_sec)]
            out.append(frag(o, qlens, ch, "mapq a mate of %d hits %s" % (H, qlens), rep_len=10))
    # 16 499 two-anchor chains masked by one primary of two anchors: n_sub + 1 = 16 500
    qlens = SE
    ch = [hit(o, qlens, 120, 20, 20 + k + 30, 50000)] + [hit(o, qlens, 30 + j % 60, 20, 20 + k + 30, 100000 + 61 * j) for j in range(16499)]
    out.append(frag(o, qlens, ch, "mapq 16500 chains, one primary"))
    return out


FAMILIES = (counts, read_lengths, primaries, selection, compaction, ties, big_scores, heavy, seg_gen, one_chain, mapq)
_CACHE = {}


def cases(optname):
    """The list of one option set (computed once per process)."""
    if optname not in _CACHE:
        o = OPTION_SETS[optname]
        out = [f for fam in FAMILIES for f in fam(o)]
        assert len({f.label for f in out}) == len(out)
        _CACHE[optname] = out
    return _CACHE[optname]


def host_only_cases(optname):
    """Fragments no batch can hold (see HOST_ONLY_READ_LENGTHS): for the comparison of the oracle with the reference alone."""
    return read_lengths(OPTION_SETS[optname], HOST_ONLY_READ_LENGTHS)


def frag_name(i):
    return b"f%d" % i


def describe(optname, f, limit=12):
    o = OPTION_SETS[optname]
    cnt = (f.u & np.uint64(0xffffffff)).astype(np.int64); off = np.concatenate([[0], np.cumsum(cnt)])
    rows = []
    for i in range(min(len(cnt), limit)):
        x, y = (int(v) for v in f.anchors[off[i]]); xe, ye = (int(v) for v in f.anchors[off[i + 1] - 1])
        rows.append("    chain %d: score %d, %d anchors, %s%d:%d q%d mate %d ... %d q%d" % (i, int(f.u[i]) >> 32, cnt[i], "-" if x >> 63 else "+", x >> 32 & 0x7fffffff, x & 0xffffffff, y & 0xffffffff, y >> 48 & 0xff,
                                                                                         xe & 0xffffffff, ye & 0xffffffff))
    return "option set %s %s\n  fragment '%s': reads %s, rep_len %d, %d chains, %d anchors\n%s%s" % (optname, tuple(o), f.label, f.qlens, f.rep_len, len(cnt), len(f.anchors), "\n".join(rows), "\n    ..." if len(cnt) > limit else "")


# ---- the reference and the oracle ----------------------------------------------------------------------------------------------------
FIELDS = ("id", "parent", "score", "score0", "cnt", "rid", "qs", "qe", "rs", "re", "subsc", "n_sub", "hash", "mlen", "blen", "rev", "sam_pri", "seg_split", "seg_id", "mapq", "other", "as")
NF = len(FIELDS)
COMPARED = tuple(n for n in FIELDS if n not in ("mapq", "as"))     # `as` is an offset into an array whose layout is each side's own: the anchors themselves are compared
Hits = namedtuple("Hits", "pre A B C anch")                      # pre: (n_u, 2) parent and `as` before the selection; A: (nA, NF); B, C: per mate (n, NF); anch: per mate (m, 2) uint64


class _Hits:
    """hitref_frag / o_frag_hits (same arguments): one fragment's chains to A, B and C."""

    def __init__(self, lib, fn):
        self.f = getattr(lib, fn); self.f.restype = C.c_int
        self.f.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint32, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float] + [C.c_int] * 6 + [C.c_void_p] * 8

    def __call__(self, o, f, hash_):
        n_u, n_a, ns = len(f.u), len(f.anchors), len(f.qlens)
        m = max(n_u, 1)
        pre = np.zeros((m, 2), dtype=np.int32); nA = np.zeros(1, dtype=np.int32); A = np.zeros((m, NF), dtype=np.int32); nB = np.zeros(2, dtype=np.int32)
        B = np.zeros((2 * m, NF), dtype=np.int32); Cc = np.zeros((2 * m, NF), dtype=np.int32); anch = np.zeros((max(n_a, 1), 2), dtype=np.uint64); n_anch = np.zeros(2, dtype=np.int64)
        ql = np.array(f.qlens, dtype=np.int32); u = np.ascontiguousarray(f.u); a = np.ascontiguousarray(f.anchors)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        rc = self.f(n_u, p(u), p(a), n_a, hash_, ns, p(ql), f.rep_len, o.mask_level, o.pri_ratio, o.best_n, 2 * o.k, max_gap_ref(o, f.qlens), 2 * o.a + o.b, o.min_chain_score, o.a,
                    p(pre), p(nA), p(A), p(nB), p(B), p(Cc), p(anch), p(n_anch))
        assert rc == 0
        Bs, Cs, an, k = [], [], [], 0
        for s in range(ns):
            Bs.append(B[s * n_u:s * n_u + nB[s]].copy()); Cs.append(Cc[s * n_u:s * n_u + nB[s]].copy())
            an.append(anch[k:k + n_anch[s]].copy()); k += int(n_anch[s])
        return Hits(pre[:n_u].copy(), A[:nA[0]].copy(), Bs, Cs, an)


def _oracle_lib():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libal_oracle.so"], check=True, capture_output=True)
    return C.CDLL(os.path.join(ROOT, "oracle", "libal_oracle.so"))


def ref_hits():
    """The reference's functions; the library is built from the reference's sources where they lie, or is the one that came with the tree."""
    p = os.path.join(ROOT, "oracle", "_ref", "libhitref.so")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "_ref/libhitref.so"], check=False, capture_output=True)
    if not os.path.exists(p):
        raise RuntimeError("oracle/_ref/libhitref.so is missing and the reference's sources are not here to build it from")
    lib = C.CDLL(p)
    assert lib.hitref_nf() == NF
    return _Hits(lib, "hitref_frag")


def oracle_hits():
    return _Hits(_oracle_lib(), "o_frag_hits")


def frag_hashes(frags):
    """The hash mm_map_frag gives fragment i of a list mapped under the name f<i> (map.c:291-293)."""
    f = _oracle_lib().o_qname_hash; f.restype = C.c_uint32; f.argtypes = [C.c_char_p, C.c_int, C.c_int]
    return [f(frag_name(i), sum(fr.qlens), SEED) for i, fr in enumerate(frags)]


_WANT = {}


def reference(optname):
    """(hashes, the reference's result for every fragment of the list), computed once per process."""
    if optname not in _WANT:
        fr = cases(optname); h = frag_hashes(fr); ref = ref_hits(); o = OPTION_SETS[optname]
        _WANT[optname] = (h, [ref(o, f, hh) for f, hh in zip(fr, h)])
    return _WANT[optname]


# ---- what a result reaches -------------------------------------------------------------------------------------------------------------
def kept_of(w):
    """(kept hits, their anchors) after chain_post."""
    return len(w.A), int(w.A[:, FIELDS.index("cnt")].sum()) if len(w.A) else 0


def heavy_tile(w, n_u):
    """The k_regs_heavy tile a fragment's kept hits fit (0 ... 4), 5 for the 9 ... 200 kept hits that fit none, None for no candidate."""
    kept, tot = kept_of(w)
    if n_u < 9 or not 9 <= kept <= 200:
        return None
    for t, (rc, ac) in enumerate(HEAVY_TILES):
        if kept <= rc and tot <= ac:
            return t
    return 5


def aliased(w):
    """The old parent indices p of the aliased tests of a fragment: a non-primary i that has more hits kept before it than parent[i] = p, whose
    parent's rank among the kept differs from p -- so that slot p holds another hit when the reference looks the parent up (hit.c:243-246)."""
    n = len(w.pre)
    if n == 0 or len(w.A) == n:
        return []
    kept_as = set(int(v) for v in w.A[:, FIELDS.index("as")])
    kept = np.array([int(w.pre[i, 1]) in kept_as for i in range(n)])
    before = np.concatenate([[0], np.cumsum(kept)[:-1]])           # hits kept before index i
    out = []
    for i in range(n):
        p = int(w.pre[i, 0])
        if p != i and before[i] > p and before[p] != p:
            out.append(p)
    return out


def n_primaries(w):
    return int((w.pre[:, 0] == np.arange(len(w.pre))).sum()) if len(w.pre) else 0


def has_tie(f, hash_):
    """Whether two chains of a fragment have equal sort keys in mm_gen_regs: equal u and equal first anchors (hit.c:62-66)."""
    cnt = (f.u & np.uint64(0xffffffff)).astype(np.int64)
    if len(cnt) < 2:
        return False
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    key = np.stack([f.u, f.anchors[first, 0], f.anchors[first, 1]], axis=1)
    return len(np.unique(key, axis=0)) < len(key)

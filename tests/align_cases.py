"""Directed fragments for the extension stage -- a mate's hits and anchors to its final records -- shared by tests/test_align_oracle_cpu.py and
tests/test_gpu_align_directed.py, and the ctypes view of what they are compared with: the reference's path from mm_gen_regs to mm_pair
(map.c:379-405: mm_align_skeleton with mm_align1, mm_update_extra, mm_filter_regs, mm_hit_sort; mm_set_parent, mm_select_sub, mm_set_sam_pri;
mm_set_mapq; mm_pair) behind oracle/alignref_shim.c (oracle/_ref/libalignref.so, built by oracle/Makefile), and the oracle's o_frag_align.

Real bases matter here: CONTIGS are four fixed random contigs -- two plain ones, a short one whose two ends the windows of align.c:613-620 reach, and
one of REP_N copies of a unit, for reads with many hits -- with a few N.  A mate is cut from a contig as a *frame* (the contig's bases in reference
direction, edited by a script of '=' copy, 'X' mismatch, 'N', 'I' insert, 'D' skip); the read in mapping orientation is the frame, or its reverse
complement for a hit on the reverse strand.  Anchors are written by hand in frame coordinates, so the generator decides where the ungapped core and
the two flanks are: mm_align1 under sr uses only the anchors' coordinates, and an anchor need not be a real minimizer match.

A fragment is (qlens, seqs, rep_len, u, anchors, label): the mates' lengths and sequences (mapping orientation: mate 2 already flipped), its chains
as u[] (score << 32 | anchors) and their anchors packed chain after chain as an (n, 2) uint64 array
    x = rev << 63 | rid << 32 | pos          y = seg << 48 | span << 32 | qpos
with qpos in the fragment's concatenated coordinates (the reverse strand: of the reversed fragment, mate 1 first), as mm_chain_dp leaves them.
Everything is deterministic; fragment i of a list is mapped under the name f<i>, which fixes its hash.  Each read length makes a batch of its own
on the device (a batch's longest read picks the LDS tile), so the families take the read length as a parameter."""
import ctypes as C
import os
import subprocess
import zlib
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

IOPT = ("k", "bw", "max_gap", "max_gap_ref", "max_frag_len", "min_cnt", "min_chain_score", "best_n", "a", "b", "q", "e", "q2", "e2", "sc_ambi", "zdrop", "zdrop_inv",
        "end_bonus", "min_dp_max", "pe_ori", "pe_bonus")
FOPT = ("mask_level", "pri_ratio", "max_clip_ratio")
Opt = namedtuple("Opt", IOPT + FOPT)
SR = Opt(21, 100, 100, -1, 800, 2, 25, 20, 2, 8, 12, 2, 24, 1, 1, 100, 100, 10, 40, 1, 33, 0.5, 0.5, 1.0)      # -ax sr (options.c)
OPTION_SETS = {
    "sr": SR,
    "end_bonus0": SR._replace(end_bonus=0),
    "zdrop30": SR._replace(zdrop=30, zdrop_inv=30),              # the z-drop cases stay short
    "min_dp_max100": SR._replace(min_dp_max=100),
    "best_n1": SR._replace(best_n=1),
    "no_closed_form": SR._replace(b=12, q=6, e=2, q2=6, e2=2),   # a + b < min(q + e, q2 + e2) fails: no flank takes the closed form
    "bw10": SR._replace(bw=10),                                  # the band runs off the matrix at short flanks
    "clip02": SR._replace(max_clip_ratio=0.2),                   # the clip filter of mm_filter_regs can fire (sr's 1.0 never lets it)
}
W = 11                                                          # the index's window (sr)
SEED = 11                                                       # mm_mapopt_t::seed
PREP_HEAVY, FIN_HEAVY, FCIG, CIG_INLINE = 8, 24, 32, 4         # the kernels' AL_PREP_HEAVY (jobs), AL_FIN_HEAVY (job slots), the words a finish lane can assemble; words a record holds itself
REP_N, REP_UNIT, REP_GAP = 24, 520, 40

Frag = namedtuple("Frag", "qlens seqs rep_len u anchors label")
Hit = namedtuple("Hit", "rev rid score pts")                    # pts: (frame position of the anchor's last base, reference position of it, span)


VAR_DIFFS = (110, 135, 160, 185, 210, 235)


def _rng(name):
    return np.random.default_rng([20251021, zlib.crc32(name.encode())])


def _contigs():
    g = _rng("contigs")
    rnd = lambda n: bytearray(b"ACGT"[c] for c in g.integers(0, 4, n))
    c0, c1, c2 = rnd(9000), rnd(5000), rnd(600)
    for p in (1000, 1001, 1500, 2222):                           # N in the reference
        c1[p] = ord("N")
    unit = rnd(REP_UNIT); rep = bytearray()
    for _ in range(REP_N):
        rep += unit + rnd(REP_GAP)
    var = bytearray(c0[1000:1400])                               # a diverged copy of a piece of c0: VAR_DIFFS substitutions
    for p in VAR_DIFFS:
        var[p] = b"ACGT"[(b"ACGT".find(bytes([var[p]])) + 1) % 4]
    return [bytes(c0), bytes(c1), bytes(c2), bytes(rep), bytes(var)]


CONTIGS = _contigs()
NAMES = [b"c0", b"c1", b"short", b"rep", b"var"]
COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def revcomp(s):
    return s.translate(COMP)[::-1]


def tile_of(o, L):
    """ext_geometry (al_kernels_align.hip): the k_align instance a batch whose longest read has L bases takes: 336, 512, 1024, or 0 for k_align_long."""
    ext = L + ((L * o.a + o.end_bonus - o.q) // o.e if L * o.a + o.end_bonus > o.q else 0)
    tb = max(2 * L + 16, ext + 16)
    return 336 if L <= 160 and tb <= 336 else 512 if L <= 256 and tb <= 512 else 1024 if L <= 512 and tb <= 1024 else 0


def tile_edges(o):
    """The longest read each of the three LDS tiles accepts, and one more."""
    out = []
    for t in (336, 512, 1024):
        L = max(l for l in range(1, 600) if tile_of(o, l) == t)
        out += [L, L + 1]
    return out


def lengths(o):
    return sorted(set([1, 15, 16, 17, 100, 150, 250] + tile_edges(o)))


LONG_L = 2000                                                    # one long-mode length, a dozen fragments at most


# ---- frames, mates, fragments ----------------------------------------------------------------------------------------------------------
def frame(g, rid, start, script):
    """The frame a script cuts from contig rid at `start`, and per frame base its reference position (-1 for an inserted base)."""
    ref = CONTIGS[rid]; out = bytearray(); pos = []; r = start
    for op, n in script:
        for _ in range(n):
            if op == "D":
                r += 1; continue
            if op == "I":
                out.append(b"ACGT"[int(g.integers(0, 4))]); pos.append(-1); continue
            assert 0 <= r < len(ref), (rid, start, script)
            b = ref[r]
            if op == "X":
                b = b"ACGT"[(b"ACGT".find(bytes([b])) + 1 + int(g.integers(0, 3))) % 4] if b != ord("N") else ord("A")
            elif op == "N":
                b = ord("N")
            out.append(b); pos.append(r); r += 1
    return bytes(out), pos


def core(pos, cs, ce, n=2, span=21):
    """n anchors of one colinear stretch over the frame interval [cs, ce): the first ends at cs + span - 1, the last at ce - 1; the diagonal is that of
    the frame base cs."""
    assert pos[cs] >= 0 and ce - cs >= span, (cs, ce, span)
    d = pos[cs] - cs
    fq = sorted(set(int(v) for v in np.linspace(cs + span - 1, ce - 1, n).round())) if n > 1 and ce - cs > span else [cs + span - 1]
    return [(q, q + d, span) for q in fq]


def hit(rev, rid, pts, score=None):
    if score is None:
        score = max(1, min(sum(p[2] for p in pts), pts[-1][0] - pts[0][0] + pts[0][2]))
    return Hit(rev, rid, score, pts)


def mate(F, rev, hits):
    """(read in mapping orientation, its hits); F is the frame of strand rev (hits on the other strand carry coordinates of the other frame)."""
    return (F if not rev else revcomp(F), hits)


def frag(mates, label, joint=True, rep_len=0):
    """The fragment of one or two mates.  joint: hit i of mate 0 and hit i of mate 1 make one chain where they lie on one contig and strand in the
    fragment's order (a pair of one chain is what the seg_fast shortcut of k_regs takes); everything else is a chain of its own."""
    qlens = tuple(len(m[0]) for m in mates); qsum = sum(qlens); chains = []

    def cat(s, rev, q):
        acc = qlens[0] if s else 0
        return q + ((qsum - (qlens[s] + acc)) if rev else acc)

    def rows(s, h):
        return [(h.rev, h.rid, r, s, cat(s, h.rev, q), sp) for q, r, sp in h.pts]
    used = [set(), set()]
    if len(mates) == 2 and joint:
        for i in range(min(len(mates[0][1]), len(mates[1][1]))):
            h0, h1 = mates[0][1][i], mates[1][1][i]
            if (h0.rev, h0.rid) != (h1.rev, h1.rid):
                continue
            first, second = ((0, h0), (1, h1)) if not h0.rev else ((1, h1), (0, h0))
            if first[1].pts[-1][1] < second[1].pts[0][1]:
                chains.append((h0.score + h1.score, rows(*first) + rows(*second))); used[0].add(i); used[1].add(i)
    for s, m in enumerate(mates):
        for i, h in enumerate(m[1]):
            if i not in used[s]:
                chains.append((h.score, rows(s, h)))
    u = np.array([(sc << 32) | len(r) for sc, r in chains], dtype=np.uint64)
    a = np.array([p for _, r in chains for p in r], dtype=np.int64).reshape(-1, 6).astype(np.uint64)
    x = a[:, 0] << np.uint64(63) | a[:, 1] << np.uint64(32) | a[:, 2]
    y = a[:, 3] << np.uint64(48) | a[:, 5] << np.uint64(32) | a[:, 4]
    return Frag(qlens, tuple(m[0] for m in mates), rep_len, u, np.ascontiguousarray(np.stack([x, y], axis=1)).reshape(-1, 2), label)


def simple(g, rid, start, script, cs, ce, rev=0, n=2, span=21, score=None):
    """One mate with one hit: the frame of the script, anchors over [cs, ce)."""
    F, pos = frame(g, rid, start, script)
    return mate(F, rev, [hit(rev, rid, core(pos, cs, ce, n, min(span, ce - cs)), score)])


def _mid(L, k=21):
    """A core in the middle of a read of L bases: [cs, ce) of at least min(k, L) bases."""
    w = min(L, max(min(k, L), L // 3))
    cs = (L - w) // 2
    return cs, cs + w


# ---- the families ---------------------------------------------------------------------------------------------------------------------
def fam_basic(o, L):
    """Every read length: exact reads on both strands, single end and as pairs of one chain and of two, a mismatch and a gap in a flank."""
    g = _rng("basic%d" % L); out = []; cs, ce = _mid(L, o.k); sp = min(o.k, ce - cs)
    for rev in (0, 1):
        out.append(frag([simple(g, 0, 700 + L, [("=", L)], cs, ce, rev, span=sp)], "exact read, single end, strand %d (%d,)" % (rev, L)))
        m0 = simple(g, 0, 1200, [("=", L)], cs, ce, rev, span=sp); m1 = simple(g, 0, 1200 + L + 60, [("=", L)], cs, ce, rev, span=sp)
        pr = [m0, m1] if not rev else [m1, m0]
        out.append(frag(pr, "exact proper pair of one chain, strand %d (%d,%d)" % (rev, L, L)))
        out.append(frag(pr, "exact proper pair of two chains, strand %d (%d,%d)" % (rev, L, L), joint=False))
        out.append(frag([pr[0], (revcomp(pr[1][0]) if L > 1 else b"N", [])], "pair with mate 2 unmapped, strand %d (%d,%d)" % (rev, L, L), joint=False))
        if L >= 40:
            for at in (2, cs - 3):
                out.append(frag([simple(g, 1, 300, [("=", at), ("X", 1), ("=", L - at - 1)], cs, ce, rev, span=sp)], "one mismatch in the left flank at %d, strand %d (%d,)" % (at, rev, L)))
            out.append(frag([simple(g, 1, 300, [("=", L - 12), ("I", 2), ("=", 10)], cs, ce, rev, span=sp)], "insertion in the right flank, strand %d (%d,)" % (rev, L)))
            out.append(frag([simple(g, 1, 300, [("=", 10), ("D", 3), ("=", L - 10)], cs + 3, ce, rev, span=min(sp, ce - cs - 3))], "deletion in the left flank, strand %d (%d,)" % (rev, L)))
    return out


def fam_windows(o, L=60):
    """align.c:613-620 on the short contig: no extension on a side, the window reaching past either contig end by -1, 0 and 1, and the branch
    l * a + end_bonus > q not taken with flanks of 0 and 1 bases and taken with 2."""
    g = _rng("windows"); out = []; n = len(CONTIGS[2]); k = o.k

    def grown(l):
        return l + ((l * o.a + o.end_bonus - o.q) // o.e if l * o.a + o.end_bonus > o.q else 0)
    for rev in (0, 1):
        out.append(frag([simple(g, 2, 0, [("=", L)], 0, 30, rev, span=k)], "core from the read's and the contig's first base: no left extension, strand %d" % rev))
        out.append(frag([simple(g, 2, n - L, [("=", L)], L - 30, L, rev, span=k)], "core to the read's and the contig's last base: no right extension, strand %d" % rev))
        out.append(frag([simple(g, 2, 100, [("=", L)], 0, L, rev, span=k)], "core over the whole read, strand %d" % rev))
        for fl in (0, 1, 2, 3, 20):
            out.append(frag([simple(g, 2, 100, [("=", L)], fl, L - fl, rev, span=k)], "flanks of %d bases, strand %d" % (fl, rev)))
        for fl in (5, 20):
            for d in (-1, 0, 1):
                st = grown(fl) - fl + d                              # rs - l = d with rs = st + fl
                if st >= 0:
                    out.append(frag([simple(g, 2, st, [("=", L)], fl, fl + 30, rev, span=k)], "left window %d bases from the contig's start, flank %d, strand %d" % (d, fl, rev)))
                st = n - L - (grown(fl) - fl) - d                    # re + l = contig length - d
                if st + L <= n:
                    out.append(frag([simple(g, 2, st, [("=", L)], L - fl - 30, L - fl, rev, span=k)], "right window %d bases from the contig's end, flank %d, strand %d" % (d, fl, rev)))
        # the read hangs over the contig's end: the query longer than the target
        F, pos = frame(g, 2, 0, [("=", L - 8)]); F = b"ACGTACGT" + F
        out.append(frag([mate(F, rev, [hit(rev, 2, [(q + 8, r, sp) for q, r, sp in core(pos, 10, 40, 2, k)])])], "left flank longer than its target, strand %d" % rev))
        F, pos = frame(g, 2, n - L + 8, [("=", L - 8)]); F = F + b"ACGTACGT"
        out.append(frag([mate(F, rev, [hit(rev, 2, core(pos, 10, 40, 2, k))])], "right flank longer than its target, strand %d" % rev))
    return out


def fam_stretch(o, L=150):
    """mm_max_stretch: one anchor, a colinear chain, a gap that leaves the longest stretch first, in the middle or last, two equal stretches."""
    g = _rng("stretch"); out = []; k = o.k
    for rev in (0, 1):
        out.append(frag([simple(g, 0, 2000, [("=", L)], 40, 40 + k, rev, n=1, span=k)], "chain of one anchor, single end: below min_cnt, loses its hit, strand %d" % rev))
        m1 = simple(g, 0, 2300, [("=", L)], 40, 100, rev, span=k)
        m0 = simple(g, 0, 2000, [("=", L)], 40, 40 + k, rev, n=1, span=k)
        out.append(frag([m0, m1] if not rev else [m1, m0], "chain of one anchor in a pair of one chain, strand %d" % rev))
        out.append(frag([simple(g, 0, 2000, [("=", L)], 20, 130, rev, n=6, span=k)], "colinear chain of six anchors, strand %d" % rev))
        for name, lens in (("first", (50, 30, 25)), ("middle", (25, 50, 30)), ("last", (25, 30, 50)), ("two equal", (40, 25, 40)), ("all equal", (30, 30, 30))):
            for gap in ("I", "D"):
                script = [("=", 5 + lens[0] + 2), (gap, 2), ("=", lens[1] + 4), (gap, 3), ("=", L)]
                F, pos = frame(g, 0, 2600, script); F = F[:L]; pos = pos[:L]
                ins = (2, 3) if gap == "I" else (0, 0)
                a0 = 5; a1 = a0 + lens[0] + 2 + ins[0] + 2; a2 = a1 + lens[1] + 2 + ins[1] + 2
                pts = core(pos, a0, a0 + lens[0], 2, k) + core(pos, a1, a1 + lens[1], 2, k) + core(pos, a2, a2 + lens[2], 2, k)
                out.append(frag([mate(F, rev, [hit(rev, 0, pts)])], "gaps (%s): the longest stretch is the %s, strand %d" % (gap, name, rev)))
        # a pair of one chain (the seg_fast shortcut) against the same chain with a second chain beside it
        m0 = simple(g, 0, 3000, [("=", L)], 30, 120, rev, n=3, span=k); m1 = simple(g, 0, 3300, [("=", L)], 30, 120, rev, n=3, span=k)
        pr = [m0, m1] if not rev else [m1, m0]
        out.append(frag(pr, "pair of one chain, strand %d" % rev))
        extra = hit(rev, 1, [(50, 700, k), (80, 730, k)], score=30)
        out.append(frag([(pr[0][0], pr[0][1] + [extra]), pr[1]], "pair of one chain with a second chain beside it, strand %d" % rev))
    return out


def fam_core(o, L=100):
    """The ungapped core: lengths 1 ... 40 at every residue mod 8 and 32, the core at every nibble phase of the packed words, both strands, mismatches,
    N in the read, in the reference and in both."""
    g = _rng("core"); out = []
    for rev in (0, 1):
        for n in range(1, 41):
            ph = (n * 3 + rev) % 8
            for cs in (ph, 32 + (ph + 5) % 8):
                m0 = simple(g, 0, 4000 + n, [("=", L)], cs, cs + n, rev, n=1 if n == 1 else 2, span=1 if n < 4 else min(n, o.k) if n % 2 else n // 2)
                m1 = simple(g, 0, 4300, [("=", L)], 30, 80, rev, span=o.k)
                out.append(frag([m0, m1] if not rev else [m1, m0], "core of %d bases from base %d in a pair of one chain, strand %d" % (n, cs, rev)))
        for n in (8, 32, 33, 64):
            for ph in range(8):
                out.append(frag([simple(g, 0, 4100 + ph, [("=", L)], ph, ph + n, rev, span=min(o.k, n))], "core of %d bases at nibble phase %d, strand %d" % (n, ph, rev)))
        for nmm in (1, 2, 5):
            sc = [("=", 20)] + [("=", 7), ("X", 1)] * nmm + [("=", L)]
            F, pos = frame(g, 0, 4500, sc)
            out.append(frag([mate(F[:L], rev, [hit(rev, 0, core(pos, 15, 85, 3, o.k))])], "%d mismatches in the core, strand %d" % (nmm, rev)))
        F, pos = frame(g, 0, 4500, [("=", 40), ("N", 2), ("=", 20), ("N", 1), ("=", L - 63)])
        out.append(frag([mate(F, rev, [hit(rev, 0, core(pos, 15, 85, 3, o.k))])], "N in the read inside the core, strand %d" % rev))
        F, pos = frame(g, 1, 960, [("=", L)])
        out.append(frag([mate(F, rev, [hit(rev, 1, core(pos, 15, 85, 3, o.k))])], "N in the reference inside the core, strand %d" % rev))
        F, pos = frame(g, 1, 960, [("=", 40), ("N", 2), ("=", 20), ("N", 1), ("=", L - 63)])
        out.append(frag([mate(F, rev, [hit(rev, 1, core(pos, 15, 85, 3, o.k))])], "N in the read and in the reference inside the core, strand %d" % rev))
        F, pos = frame(g, 1, 1460, [("=", 10), ("N", 1), ("=", L - 11)])
        out.append(frag([mate(F, rev, [hit(rev, 1, core(pos, 50, 90, 2, o.k))])], "N in both in the left flank, strand %d" % rev))
    return out


def _drop_block(o, drop):
    """A run of mismatches and N whose score falls by exactly `drop` along the diagonal (mismatch -b, N -sc_ambi)."""
    nm = drop // o.b
    return [("X", nm), ("N", (drop - nm * o.b) // o.sc_ambi)]


def fam_zdrop(o, L=250):
    """z-drop in the core: a fall of exactly zdrop and of one more; a fall the second pass aligns through with a gap; falls that split the hit with
    cnt1 - (j + 1) = min_cnt - 1 and min_cnt.  (mm_test_zdrop never returns 2 under sr: align.c:72.)"""
    g = _rng("zdrop"); out = []; k = o.k; z = o.zdrop
    for rev in (0, 1):
        for d in (z - 1, z, z + 1, z + 2 * o.b):
            for after in (1, 2, 3):                                       # anchors behind the fall
                blk = _drop_block(o, d); nb = sum(n for _, n in blk)
                head = 60; tail = L - 10 - head - nb
                if tail < 3 * k:
                    continue
                F, pos = frame(g, 0, 5000, [("=", 10 + head)] + blk + [("=", tail)])
                pts = core(pos, 10, 10 + head, 2, k) + [(q, q + pos[10] - 10, k) for q in np.linspace(10 + head + nb + k, L - 11, after).round().astype(int).tolist()]
                out.append(frag([mate(F, rev, [hit(rev, 0, pts)])], "fall of %d in the core (zdrop %d), %d anchors behind it, strand %d" % (d, z, after, rev)))
        for n in ((60, 90) if z > 50 else (20, 30)):                        # too far apart for a gap to bridge: the second pass drops too
            for after in (1, 2, 3):
                F, pos = frame(g, 0, 5200, [("=", 70), ("I", n), ("D", n), ("=", L)]); F = F[:L]; pos = pos[:L]
                pts = core(pos, 10, 60, 2, k) + [(q, q + pos[10] - 10, k) for q in np.linspace(70 + n + k + 5, L - 11, after).round().astype(int).tolist()]
                out.append(frag([mate(F, rev, [hit(rev, 0, pts)])], "%d bases of the read replaced inside the core, %d anchors behind them: the hit is cut%s, strand %d" % (n, after, " and split" if after >= o.min_cnt else "", rev)))
                m1 = simple(g, 0, 5200 + 400, [("=", 150)], 40, 110, rev, span=k)
                m0 = mate(F, rev, [hit(rev, 0, pts)])
                out.append(frag([m0, m1] if not rev else [m1, m0], "%d bases of mate 1 replaced inside the core, %d anchors behind them, pair of one chain, strand %d" % (n, after, rev)))
        for gap, n in (("I", 3), ("D", 3), ("D", 12)):
            # (a gap dearer than zdrop would drop in the second pass too and split; the second hit's anchors then lie on a diagonal its bases do not follow, its
            # core drops before a base aligns, and with an empty left flank the reference reads r->p == NULL at align.c:747 -- real anchors match their bases)
            if min(o.q + o.e * n, o.q2 + o.e2 * n) > z:
                continue
            F, pos = frame(g, 0, 5400, [("=", 80), (gap, n), ("=", L)]); F = F[:L]; pos = pos[:L]
            pts = [(q, q + pos[10] - 10, k) for q in (10 + k - 1, 60, L - 40, L - 11)]
            out.append(frag([mate(F, rev, [hit(rev, 0, pts)])], "a gap (%s%d) inside the core: the fall the second pass aligns through, strand %d" % (gap, n, rev)))
    return out


def fam_flanks(o, L=100):
    """The flanks: exact, one mismatch at every position (the closed form), two mismatches, N, gaps at 1, 2 and 10 bases from the end, a soft clip
    against the end bonus, ends that tie with the end bonus."""
    g = _rng("flanks%d" % L); out = []; k = o.k; fl = 30; cs, ce = fl, L - fl
    assert ce - cs >= k
    for rev in (0, 1):
        for p in list(range(0, fl)):
            out.append(frag([simple(g, 0, 6000, [("=", p), ("X", 1), ("=", L - p - 1)], cs, ce, rev, span=k)], "one mismatch at base %d of the left flank, strand %d" % (p, rev)))
            out.append(frag([simple(g, 0, 6000, [("=", L - p - 1), ("X", 1), ("=", p)], cs, ce, rev, span=k)], "one mismatch %d bases before the end of the right flank, strand %d" % (p, rev)))
        for p, q in ((0, 1), (3, 4), (3, 7), (0, 5), (10, 20), (27, 28)):
            out.append(frag([simple(g, 0, 6000, [("=", p), ("X", 1), ("=", q - p - 1), ("X", 1), ("=", L - q - 1)], cs, ce, rev, span=k)], "two mismatches at %d and %d of the left flank, strand %d" % (p, q, rev)))
            out.append(frag([simple(g, 0, 6000, [("=", L - q - 1), ("X", 1), ("=", q - p - 1), ("X", 1), ("=", p)], cs, ce, rev, span=k)], "two mismatches %d and %d before the read's end, strand %d" % (q, p, rev)))
        for p in (0, 5, 29):
            out.append(frag([simple(g, 0, 6000, [("=", p), ("N", 1), ("=", L - p - 1)], cs, ce, rev, span=k)], "N at base %d of the left flank, strand %d" % (p, rev)))
            out.append(frag([simple(g, 0, 6000, [("=", L - p - 1), ("N", 1), ("=", p)], cs, ce, rev, span=k)], "N %d bases before the read's end, strand %d" % (p, rev)))
        for d in (1, 2, 10):
            for gap, n in (("I", 1), ("I", 4), ("D", 1), ("D", 4)):
                ins = n if gap == "I" else 0
                out.append(frag([simple(g, 0, 6000, [("=", d), (gap, n), ("=", L - d - ins)], cs + ins if gap == "I" else cs, ce, rev, span=k)], "%s%d %d bases from the read's start, strand %d" % (gap, n, d, rev)))
                out.append(frag([simple(g, 0, 6000, [("=", L - d - ins), (gap, n), ("=", d)], cs, ce - ins if gap == "I" else ce, rev, span=k)], "%s%d %d bases before the read's end, strand %d" % (gap, n, d, rev)))
        for nx in (2, 3, 6, 12):
            out.append(frag([simple(g, 0, 6000, [("X", nx), ("=", L - nx)], cs, ce, rev, span=k)], "%d mismatches at the read's start: soft clip against the end bonus, strand %d" % (nx, rev)))
            out.append(frag([simple(g, 0, 6000, [("=", L - nx), ("X", nx)], cs, ce, rev, span=k)], "%d mismatches at the read's end: soft clip against the end bonus, strand %d" % (nx, rev)))
        for nx in (1, 2):                                                     # sc + end_bonus against mx: t matching bases behind nx mismatches
            for t in range(0, 9):
                out.append(frag([simple(g, 0, 6000, [("=", L - nx - t), ("X", nx), ("=", t)], cs, ce, rev, span=k)], "%d mismatches and %d matches at the read's end: the reach-end tie, strand %d" % (nx, t, rev)))
                out.append(frag([simple(g, 0, 6000, [("=", t), ("X", nx), ("=", L - nx - t)], cs, ce, rev, span=k)], "%d matches and %d mismatches at the read's start: the reach-end tie, strand %d" % (t, nx, rev)))
    return out


def fam_runoff(o, L):
    """A flank whose target is bw * 1.5 + 1 and one more longer than the query (the band runs off the matrix: the closed form flags it like a z-drop),
    and a z-drop inside a flank."""
    g = _rng("runoff%d" % L); out = []; k = o.k; wb = int(o.bw * 1.5 + 1.)

    def grown(l):
        return l + ((l * o.a + o.end_bonus - o.q) // o.e if l * o.a + o.end_bonus > o.q else 0)
    for rev in (0, 1):
        for fl in range(2, L - k):
            if grown(fl) - fl in (wb - 1, wb, wb + 1, wb + 2):
                for mm in (0, 1):
                    out.append(frag([simple(g, 0, 6500, [("=", fl // 2), ("X", mm), ("=", L - fl // 2 - mm)], fl, min(L, fl + 40), rev, span=k)], "left flank of %d bases, target %d longer (band %d), %d mismatches, strand %d" % (fl, grown(fl) - fl, wb, mm, rev)))
                    out.append(frag([simple(g, 0, 6500, [("=", L - fl // 2 - mm), ("X", mm), ("=", fl // 2)], max(0, L - fl - 40), L - fl, rev, span=k)], "right flank of %d bases, target %d longer (band %d), %d mismatches, strand %d" % (fl, grown(fl) - fl, wb, mm, rev)))
        for d in (o.zdrop, o.zdrop + 1, o.zdrop + 3 * o.b):
            blk = _drop_block(o, d); nb = sum(n for _, n in blk)
            if 30 + k + 20 + nb + 40 <= L:
                out.append(frag([simple(g, 0, 6500, [("=", 30 + k + 20)] + blk + [("=", L - 30 - k - 20 - nb)], 30, 30 + k, rev, span=k)], "fall of %d inside the right flank, strand %d" % (d, rev)))
                out.append(frag([simple(g, 0, 6500, [("=", L - 30 - k - 20 - nb)] + blk + [("=", 30 + k + 20)], L - 30 - k, L - 30, rev, span=k)], "fall of %d inside the left flank, strand %d" % (d, rev)))
    return out


def _gappy(n_gaps, L, at=8, step=12):
    """A script of L frame bases with n_gaps alternating 1-base insertions and deletions, `step` apart, from base `at` on."""
    sc = [("=", at)]; used = at
    for i in range(n_gaps):
        sc.append(("I", 1) if i % 2 == 0 else ("D", 1)); used += 1 - i % 2
        sc.append(("=", step)); used += step
    assert used <= L, (n_gaps, L)
    return sc + [("=", L - used)]


def fam_cigar(o, L=250):
    """CIGAR assembly: flanks with so many gaps that left + core + right come to 31 ... 35 words around the 32 a finish lane can assemble; more than CIG_INLINE words; a flank's M
    merging with the core's and not (a gap right beside the core); an empty left flank CIGAR."""
    g = _rng("cigar"); out = []; k = o.k
    for rev in (0, 1):
        for ng in (1, 2, 3, 6, 12, 13, 14, 15, 16, 17):
            sc = _gappy(ng, L); F, pos = frame(g, 0, 7000, sc)
            cs = next(i for i in range(L - 30 - k, L) if pos[i] >= 0)
            out.append(frag([mate(F, rev, [hit(rev, 0, core(pos, cs, cs + k, 1, k) + core(pos, cs + 3, cs + 3 + k, 1, k))])], "%d gaps in the left flank, core at the read's end, strand %d" % (ng, rev)))
            sc = _gappy(ng, L, at=30); F, pos = frame(g, 0, 7000, sc)
            out.append(frag([mate(F, rev, [hit(rev, 0, core(pos, 5, 5 + k + 3, 2, k))])], "%d gaps in the right flank, core at the read's start, strand %d" % (ng, rev)))
            if ng <= 8:
                sc = _gappy(ng, 100, at=8) + [("=", 50)] + _gappy(ng, 100, at=8); F, pos = frame(g, 0, 7000, sc)
                out.append(frag([mate(F, rev, [hit(rev, 0, core(pos, 110, 140, 2, k))])], "%d gaps in either flank, strand %d" % (ng, rev)))
        # exactly FCIG words, the most a finish lane's buffer holds: 14 single-base gaps (29 words) and n bases replaced, which the DP takes as one I and one D (and
        # one more M) where no part of the replacement happens to match -- the two seeds are the first of a search for which the reference does (under sr; the
        # CPU test asserts that the count is reached)
        n = 24; sc = _gappy(14, 183, at=8) + [("I", n), ("D", n), ("=", L - 183 - n)]; F, pos = frame(_rng("cigar32_29"), 0, 7000, sc)
        out.append(frag([mate(F, rev, [hit(rev, 0, core(pos, L - 5 - k - 3, L - 5, 2, k))])], "a CIGAR of exactly %d words from the left flank, strand %d" % (FCIG, rev)))
        n = 22; pre = 5 + k + 3 + 10; sc = [("=", pre), ("I", n), ("D", n)] + _gappy(14, L - n - pre, at=8); F, pos = frame(_rng("cigar32_7"), 0, 7000, sc)
        out.append(frag([mate(F, rev, [hit(rev, 0, core(pos, 5, 5 + k + 3, 2, k))])], "a CIGAR of exactly %d words from the right flank, strand %d" % (FCIG, rev)))
        for gap in ("I", "D"):
            F, pos = frame(g, 0, 7300, [("=", 99), (gap, 2), ("=", L)]); F = F[:L]; pos = pos[:L]
            c0 = 99 + (2 if gap == "I" else 0)
            out.append(frag([mate(F, rev, [hit(rev, 0, core(pos, c0, c0 + 40, 2, k))])], "a gap (%s) right before the core: the left flank's CIGAR does not end in M, strand %d" % (gap, rev)))
            out.append(frag([mate(F, rev, [hit(rev, 0, core(pos, 50, 99, 2, k))])], "a gap (%s) right behind the core: the right flank's CIGAR does not begin with M, strand %d" % (gap, rev)))
        out.append(frag([simple(g, 0, 7300, [("X", 12), ("=", L - 12)], 12, 80, rev, span=k)], "left flank all mismatches: its CIGAR is empty, strand %d" % rev))
        out.append(frag([simple(g, 0, 7300, [("X", 4), ("=", L - 4)], 4, 80, rev, span=k)], "left flank of four mismatches, strand %d" % rev))
    return out


def _rep_start(c):
    return c * (REP_UNIT + REP_GAP)


def rep_mate(g, L, copies, rev, off=0, script=None, cs=None, ce=None, k=21, scores=None):
    """A mate cut from the unit of the repeat contig with a hit on each of `copies`."""
    F, pos = frame(g, 3, _rep_start(copies[0]) + off, script or [("=", L)])
    F = F[:L]; pos = pos[:L]
    if cs is None:
        cs, ce = _mid(L, k)
    pts0 = core(pos, cs, ce, 2, min(k, ce - cs))
    hits = [hit(rev, 3, [(q, r + _rep_start(c) - _rep_start(copies[0]), sp) for q, r, sp in pts0], None if scores is None else scores[i]) for i, c in enumerate(copies)]
    return mate(F, rev, hits)


def fam_hits(o, L):
    """1, 3, 4, 12 and more hits per mate on the repeat contig: both sides of AL_PREP_HEAVY (8 jobs) and AL_FIN_HEAVY (24 slots); best_n reached;
    hits that become identical by alignment; a hit that needs the monolithic kernel as hit 0, 1 or last of a wave-form fragment."""
    g = _rng("hits%d" % L); out = []; k = o.k
    if L < 30 or L > REP_UNIT - 10:
        return out
    for rev in (0, 1):
        for n in (1, 3, 4, 5, 11, 12, 13, REP_N):
            cp = list(range(n))
            out.append(frag([rep_mate(g, L, cp, rev, k=k)], "%d hits, single end, strand %d (%d,)" % (n, rev, L)))
            m0 = rep_mate(g, L, cp, rev, off=0, k=k); m1 = rep_mate(g, L, cp, rev, off=REP_UNIT - L, k=k)
            if L <= REP_UNIT // 2 - 5:
                out.append(frag([m0, m1] if not rev else [m1, m0], "%d x %d hits, pair of joint chains, strand %d (%d,%d)" % (n, n, rev, L, L)))
                out.append(frag([m0, m1] if not rev else [m1, m0], "%d x %d hits, pair of separate chains, strand %d (%d,%d)" % (n, n, rev, L, L), joint=False))
        # descending scores: the k-th hit by score is the one with a gap inside its core -> the ungapped core z-drops there only if the copies differ; here every
        # copy is alike, so the slow hit is made by an anchor set of its own: a core across an insertion
        if L >= 150:
            F, pos = frame(g, 3, 0, [("=", 70), ("I", 3), ("=", L)]); F = F[:L]; pos = pos[:L]
            good = core(pos, 80, 80 + 40, 2, k)
            bad = [(q, q + pos[10] - 10, k) for q in (10 + k - 1, 60, L - 40, L - 11)]        # a core over the insertion: mm_test_zdrop fires
            for n in (12, 13):
                for kth in (0, 1, n - 1):
                    sc = [400 - 5 * i for i in range(n)]
                    hs = [hit(rev, 3, [(q, r + _rep_start(c), sp) for q, r, sp in (bad if c == kth else good)], sc[c]) for c in range(n)]
                    out.append(frag([mate(F, rev, hs)], "%d hits, hit %d is the first that needs the monolithic kernel, strand %d (%d,)" % (n, kth, rev, L)))
        # two chains that align to the same record
        F, pos = frame(g, 0, 7600, [("=", L)])
        h0 = hit(rev, 0, core(pos, 5, 5 + 30, 2, k), 60); h1 = hit(rev, 0, core(pos, L - 40, L - 5, 2, k), 50)
        out.append(frag([mate(F, rev, [h0, h1])], "two chains of one diagonal: identical after alignment, strand %d (%d,)" % (rev, L)))
    return out


def fam_pairs(o, L=150):
    """mm_pair: proper pairs, the mates max_gap_ref apart and one more, wrong orientation, different contigs, a mate of two equal hits of which the
    pair picks the one beside the other mate (the primary moves), pe_thru, a grid of hits."""
    g = _rng("pairs"); out = []; k = o.k
    mg = o.max_gap_ref if o.max_gap_ref > 0 else max(o.max_frag_len - 2 * L, o.max_gap) if o.max_frag_len > 0 else o.max_gap
    cs, ce = _mid(L, k)
    for rev in (0, 1):
        for d in (0, 50, mg - 1, mg, mg + 1, mg + 200):
            for joint in (True, False):
                a = simple(g, 0, 1000, [("=", L)], cs, ce, rev, span=k); b = simple(g, 0, 1000 + L + d, [("=", L)], cs, ce, rev, span=k)
                out.append(frag([a, b] if not rev else [b, a], "mates %d bases apart (max_gap_ref %d), %s, strand %d" % (d, mg, "one chain" if joint else "two chains", rev), joint=joint))
        a = simple(g, 0, 1000, [("=", L)], cs, ce, rev, span=k); b = simple(g, 0, 1400, [("=", L)], cs, ce, 1 - rev, span=k)
        out.append(frag([a, b], "mates on opposite strands in mapping orientation, strand %d" % rev))
        out.append(frag([b, a], "mates on opposite strands in mapping orientation, swapped, strand %d" % rev))
        a = simple(g, 0, 1400, [("=", L)], cs, ce, rev, span=k); b = simple(g, 0, 1000, [("=", L)], cs, ce, rev, span=k)
        out.append(frag([a, b] if not rev else [b, a], "mates in the wrong order, strand %d" % rev, joint=False))
        a = simple(g, 0, 1000, [("=", L)], cs, ce, rev, span=k); b = simple(g, 1, 1200, [("=", L)], cs, ce, rev, span=k)
        out.append(frag([a, b], "mates on different contigs, strand %d" % rev))
        # pe_thru: both mates over the same interval
        for d in (0, 2, 3):
            a = simple(g, 0, 1000, [("=", L)], cs, ce, rev, span=k); b = simple(g, 0, 1000 + d, [("=", L)], cs, ce, rev, span=k)
            out.append(frag([a, b] if not rev else [b, a], "mates over one interval, %d bases shifted (pe_thru), strand %d" % (d, rev), joint=False))
        # the pair bonus: mate 0 has a better hit far away (fewer mismatches) and a worse one beside mate 1
        for nmm in (1, 2, 3, 4):
            unit0 = _rep_start(2)
            F, pos = frame(g, 3, unit0, [("=", 10)] + [("X", 1), ("=", 9)] * nmm + [("=", L)]); F = F[:L]; pos = pos[:L]
            cs2 = 10 + 10 * nmm + 5
            pts = core(pos, cs2, cs2 + 40, 2, k)
            m0 = mate(F, rev, [hit(rev, 3, [(q, r + _rep_start(c) - unit0, sp) for q, r, sp in pts], 60) for c in (2, 9)])
            G1, p1 = frame(g, 3, _rep_start(9 if not rev else 8) + REP_UNIT - 60, [("=", L)])
            m1 = mate(G1, rev, [hit(rev, 3, core(p1, cs, ce, 2, k), 60)])
            out.append(frag([m0, m1] if not rev else [m1, m0], "mate 1 of two equal hits, mate 2 beside one of them, %d mismatches, strand %d" % (nmm, rev), joint=False))
        # a grid: n x n hits on the repeat
        for n in (2, 5, 20):
            m0 = rep_mate(g, L, list(range(n)), rev, off=0, k=k); m1 = rep_mate(g, L, list(range(n)), rev, off=REP_UNIT - L - 20, k=k)
            out.append(frag([m0, m1] if not rev else [m1, m0], "%d x %d grid of hits, strand %d" % (n, n, rev), joint=False))
            out.append(frag([m0, m1] if not rev else [m1, m0], "%d x %d grid of hits, joint chains, strand %d" % (n, n, rev)))
    return out


def fam_filter(o):
    """mm_update_extra and mm_filter_regs: reads short enough to fall below min_chain_score matching bases and min_dp_max, with and without mismatches; a
    negative tail (dp_max above dp_score); n_ambi; fragments that lose every hit."""
    g = _rng("filter"); out = []; k = o.k
    lo = max(k + 1, o.min_dp_max // o.a - 8)
    for rev in (0, 1):
        for L in range(lo, o.min_dp_max // o.a + 12):
            for nmm in (0, 1):
                cs = (L - k) // 2
                sc = [("=", 2), ("X", nmm), ("=", L - 2 - nmm)]
                out.append(frag([simple(g, 0, 8000, sc, cs, cs + k, rev, n=2, span=k - 1)], "read of %d bases, %d mismatches: around min_dp_max %d, strand %d (%d,)" % (L, nmm, o.min_dp_max, rev, L)))
            if L >= 26:                                                       # two mismatches (and an N) inside the core: the running score is never clamped, dp_max = a * matches - b * 2 (- sc_ambi)
                for nn in (0, 1):
                    sc = [("=", 12), ("X", 1), ("=", 7), ("X", 1), ("N", nn), ("=", L - 21 - nn)]
                    out.append(frag([simple(g, 0, 8000, sc, 1, L - 1, rev, n=2, span=k)], "read of %d bases, two mismatches and %d N in the core: around min_dp_max %d, strand %d (%d,)" % (L, nn, o.min_dp_max, rev, L)))
    return out


def fam_clip(o, L=100):
    """The clip filter of mm_filter_regs (both ends clipped by more than qlen * max_clip_ratio): c mismatching bases at either end are soft-clipped exactly, c on
    each side of the bound and one end on each side of it."""
    g = _rng("clip"); out = []; k = o.k; b = int(L * min(o.max_clip_ratio, 0.3))
    for rev in (0, 1):
        for cl, cr in ((b - 1, b - 1), (b, b), (b + 1, b + 1), (b + 2, b + 2), (b + 1, b), (b, b + 1), (b + 1, 0), (b + 5, b + 1)):
            sc = [("X", cl), ("=", L - cl - cr), ("X", cr)]
            out.append(frag([simple(g, 0, 8300, sc, 40, 60 + k - 20, rev, span=k)], "%d and %d bases clipped of %d (bound %d), strand %d" % (cl, cr, L, b, rev)))
    return out


def fam_parent(o, L=150):
    """A parent change after mm_hit_sort: the chain with the higher chaining score lies on the diverged copy and aligns worse, so the sort by dp_max puts the
    other chain first and the primary moves."""
    g = _rng("parent"); out = []; k = o.k; cs, ce = _mid(L, k)
    for rev in (0, 1):
        for hi, lo in ((200, 100), (120, 119)):
            F, pos = frame(g, 0, 1100, [("=", L)])
            pts = core(pos, cs, ce, 2, k)
            better = hit(rev, 0, pts, lo); worse = hit(rev, 4, [(q, r - 1000, sp) for q, r, sp in pts], hi)
            out.append(frag([mate(F, rev, [worse, better])], "the higher chain score aligns worse (%d against %d): the parent changes after the sort, strand %d" % (hi, lo, rev)))
            m1 = simple(g, 0, 1100 + L + 80, [("=", L)], cs, ce, rev, span=k)
            m0 = mate(F, rev, [worse, better])
            out.append(frag([m0, m1] if not rev else [m1, m0], "the higher chain score aligns worse (%d against %d), in a pair, strand %d" % (hi, lo, rev), joint=False))
    return out


def fam_long(o):
    """A dozen fragments of LONG_L bases: k_align_long."""
    g = _rng("long"); out = []; L = LONG_L; k = o.k
    for rev in (0, 1):
        out.append(frag([simple(g, 0, 3000, [("=", L)], 900, 1100, rev, n=4, span=k)], "long exact read, strand %d (%d,)" % (rev, L)))
        out.append(frag([simple(g, 0, 3000, _gappy(20, L, at=100, step=40), 1200, 1300, rev, n=3, span=k)], "long read with 20 gaps in the left flank, strand %d (%d,)" % (rev, L)))
        out.append(frag([simple(g, 0, 3000, [("=", 1500), ("X", 1), ("=", 200), ("I", 2), ("=", L - 1703)], 900, 1100, rev, n=4, span=k)], "long read with a mismatch and a gap in the right flank, strand %d (%d,)" % (rev, L)))
        a = simple(g, 0, 500, [("=", L)], 900, 1100, rev, n=4, span=k); b = simple(g, 0, 2800, [("=", L)], 900, 1100, rev, n=4, span=k)
        out.append(frag([a, b] if not rev else [b, a], "long pair, strand %d (%d,%d)" % (rev, L, L)))
    return out


def fam_arena(o, L=250, n=24):
    """Enough long CIGARs in one small batch that the CIGAR arena overflows once: n reads with a hit of more than 30 CIGAR words on each of 20 copies."""
    g = _rng("arena"); out = []
    sc = _gappy(15, L, at=8, step=12)
    for i in range(n):
        rev = i & 1
        F, pos = frame(g, 3, 0, sc); F = F[:L]; pos = pos[:L]
        cs = next(j for j in range(L - 30 - o.k, L) if pos[j] >= 0)
        pts = core(pos, cs, cs + o.k, 1, o.k) + core(pos, cs + 3, cs + 3 + o.k, 1, o.k)
        hs = [hit(rev, 3, [(q, r + _rep_start(c), sp) for q, r, sp in pts], 100) for c in range(20)]
        out.append(frag([mate(F, rev, hs)], "arena: 20 hits of 15 gaps each, read %d (%d,)" % (i, L)))
    return out


_CASES = {}


def cases(optname):
    """The fragments of an option set (the arena batch and the long-mode batch are lists of their own: arena_cases, long_cases)."""
    if optname in _CASES:
        return _CASES[optname]
    o = OPTION_SETS[optname]; out = []
    for L in lengths(o):
        out += fam_basic(o, L) + fam_hits(o, L)
    out += fam_windows(o) + fam_stretch(o) + fam_core(o) + fam_flanks(o) + fam_cigar(o) + fam_pairs(o) + fam_filter(o) + fam_clip(o) + fam_parent(o)
    out += fam_zdrop(o, 250 if o.zdrop > 50 else 150)
    for L in (100, 250):
        out += fam_runoff(o, L)
    _CASES[optname] = out
    return out


def long_cases(optname):
    return fam_long(OPTION_SETS[optname])


def arena_cases(optname):
    return fam_arena(OPTION_SETS[optname])


def frag_name(i):
    return b"f%d" % i


def describe(optname, f):
    rows = []; cnt = (f.u & np.uint64(0xffffffff)).astype(np.int64); off = np.concatenate([[0], np.cumsum(cnt)])
    for i in range(min(len(cnt), 4)):
        a = f.anchors[off[i]:off[i + 1]]
        rows.append("    chain %d: score %d: %s" % (i, int(f.u[i]) >> 32, " ".join("%s%d:%d/q%d.%d+%d" % ("-" if int(x) >> 63 else "+", int(x) >> 32 & 0x7fffffff, int(x) & 0xffffffff, int(y) >> 48 & 0xff, int(y) & 0xffffffff, int(y) >> 32 & 0xff) for x, y in a[:8])))
    return "option set %s\n  fragment '%s': reads %s, %d chains\n%s" % (optname, f.label, f.qlens, len(cnt), "\n".join(rows))


# ---- the reference and the oracle ----------------------------------------------------------------------------------------------------
FIELDS = ("id", "parent", "score", "score0", "cnt", "rid", "qs", "qe", "rs", "re", "subsc", "n_sub", "hash", "mlen", "blen", "mapq", "rev", "split", "inv", "split_inv", "proper_frag",
          "pe_thru", "sam_pri", "seg_split", "seg_id", "has_p", "dp_score", "dp_max", "dp_max2", "n_ambi", "trans_strand", "n_cigar")
NF = len(FIELDS)
COL = {n: i for i, n in enumerate(FIELDS)}
AC = ("align1", "stretch_first", "stretch_mid", "stretch_last", "win_grown", "win_plain", "win_left_at0", "win_left_cut", "win_right_at_end", "win_right_cut", "left", "right", "flank_zdrop",
      "reach_end", "clipped", "flank_empty", "core_zdrop", "core_second_pass_kept", "split", "drop_no_split", "flt_mlen", "flt_dp", "flt_dp_just_below", "flt_clip", "flt_clip_just_above",
      "kept_at_min_dp", "kept_clip_at_bound", "fall_eq_zdrop", "fall_zdrop_plus1", "cigar_merged", "cigar_not_merged", "tie_eq", "tie_above", "select_dropped")
Result = namedtuple("Result", "hits cigars")                     # per mate: (n, NF) int32; per mate: list of uint32 arrays


class _Align:
    """alignref_frag / o_frag_align (same arguments) on an index of CONTIGS."""
    MAX_HITS, MAX_CIG = 256, 65536

    def __init__(self, lib, prefix, k):
        p = C.c_void_p
        self.f = getattr(lib, prefix + "frag" if prefix == "alignref_" else "o_frag_align"); self.f.restype = C.c_int
        self.f.argtypes = [p, p, p, C.c_int, p, p, C.c_int64, C.c_uint32, C.c_int, p, p, C.c_int, C.c_int, C.c_int, p, p, p, p]
        mk = getattr(lib, "alignref_idx" if prefix == "alignref_" else "o_align_idx"); mk.restype = p; mk.argtypes = [C.c_int, C.c_int, C.c_int, p, p]
        self.free = getattr(lib, "alignref_idx_free" if prefix == "alignref_" else "o_align_idx_free"); self.free.argtypes = [p]
        n = len(CONTIGS); self._s = (C.c_char_p * n)(*CONTIGS); self._n = (C.c_char_p * n)(*NAMES)
        self.mi = mk(W, k, n, self._s, self._n)
        assert self.mi
        self.out = np.zeros((2 * self.MAX_HITS, NF), dtype=np.int32); self.cig = np.zeros(2 * self.MAX_CIG, dtype=np.uint32)

    def __call__(self, o, f, hash_):
        ns = len(f.qlens); nh = np.zeros(2, dtype=np.int32); nc = np.zeros(2, dtype=np.int32)
        io = np.array([getattr(o, n) for n in IOPT], dtype=np.int32); fo = np.array([getattr(o, n) for n in FOPT], dtype=np.float32)
        ql = np.array(f.qlens, dtype=np.int32); sq = (C.c_char_p * ns)(*f.seqs); u = np.ascontiguousarray(f.u); a = np.ascontiguousarray(f.anchors)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        rc = self.f(self.mi, p(io), p(fo), len(u), p(u), p(a), len(a), hash_, ns, p(ql), C.cast(sq, C.c_void_p), f.rep_len, self.MAX_HITS, self.MAX_CIG, p(nh), p(self.out), p(nc), p(self.cig))
        assert rc == 0, "%s: return code %d" % (f.label, rc)
        hits, cigs = [], []
        for s in range(ns):
            h = self.out[s * self.MAX_HITS:s * self.MAX_HITS + nh[s]].copy(); hits.append(h)
            w = self.cig[s * self.MAX_CIG:s * self.MAX_CIG + nc[s]]; off = np.concatenate([[0], np.cumsum(h[:, COL["n_cigar"]])]) if len(h) else [0]
            cigs.append([w[off[i]:off[i + 1]].copy() for i in range(len(h))])
        return Result(hits, cigs)


def _oracle_lib():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libal_oracle.so"], check=True, capture_output=True)
    return C.CDLL(os.path.join(ROOT, "oracle", "libal_oracle.so"))


def ref_align(k=21):
    """The reference's functions; the library is built from the reference's sources where they lie, or is the one that came with the tree."""
    p = os.path.join(ROOT, "oracle", "_ref", "libalignref.so")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "_ref/libalignref.so"], check=False, capture_output=True)
    if not os.path.exists(p):
        raise RuntimeError("oracle/_ref/libalignref.so is missing and the reference's sources are not here to build it from")
    lib = C.CDLL(p)
    assert lib.alignref_nf() == NF and lib.alignref_ni() == len(IOPT)
    return _Align(lib, "alignref_", k)


def oracle_align(k=21):
    return _Align(_oracle_lib(), "o_", k)


def oracle_count(counters):
    """Point the oracle's branch counters (AC) at an int64 array, or at nothing."""
    f = _oracle_lib().o_align_count; f.argtypes = [C.c_void_p]; f.restype = None
    f(None if counters is None else counters.ctypes.data_as(C.c_void_p))


def frag_hashes(frags):
    f = _oracle_lib().o_qname_hash; f.restype = C.c_uint32; f.argtypes = [C.c_char_p, C.c_int, C.c_int]
    return [f(frag_name(i), sum(fr.qlens), SEED) for i, fr in enumerate(frags)]


_WANT = {}


def reference(optname, which="cases"):
    """(hashes, the reference's result for every fragment of a list), computed once per process."""
    key = (optname, which)
    if key not in _WANT:
        fr = {"cases": cases, "long": long_cases, "arena": arena_cases}[which](optname); h = frag_hashes(fr); o = OPTION_SETS[optname]; ref = ref_align(o.k)
        _WANT[key] = (h, [ref(o, f, hh) for f, hh in zip(fr, h)])
    return _WANT[key]

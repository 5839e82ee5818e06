"""Directed cases for the sketch, seed-lookup and anchor stages (K1 ... K3), shared by tests/test_seed_oracle_cpu.py and tests/test_gpu_seed_directed.py,
and a ctypes view of the reference they are compared with: mm_sketch, mm_idx_str and the static collect_minimizers / collect_seed_hits_heap of the
fork's map.c, compiled behind oracle/seedref_shim.c as oracle/_ref/libseedref.so by oracle/Makefile.

A case set is (shape, contigs, fragments, second-pass list).  The shape fixes the contig count, k, w and the two occurrence bounds (mid_occ for the
first pass, max_occ for the re-chain pass; both far below the preset's so that a reference of a megabase holds lists at and above them).  Everything
is generated from random generators seeded by the case's name.  The reference is made of repeat families -- a unit copied c times over the long
contigs, on both strands, between unique spacers -- plus a unique region U.  A fragment is a few pieces of family units (its bulk: one minimizer
of a unit's interior gives c anchors), optionally a piece that occurs twice in the fragment (equal x: a tied fragment), and a tail copied from U
whose minimizers add one anchor each; the tail is trimmed until the reference library reports exactly the wanted anchor or list count (fit()).

A fragment's sequences are kept in MAPPING orientation, as the reference's map.c sees them after worker_for flipped mate 2; upload_reads() gives
what a batch upload takes (mate 2 as read, i.e. the reverse complement; the device flips it back).

Not generated, because it cannot occur: a tied fragment of ONE list (positions inside an occurrence list are distinct, and a list's anchors share
the query strand); repeat intervals nested in each other (map.c:105-111: every minimizer of this index has span k and they come in ascending
position, so an interval never ends before its predecessor does); fragments of three segments (al_batch_upload accepts one or two)."""
import ctypes as C
import hashlib
import os
import subprocess
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMP = bytes.maketrans(b"ACGTUMRWSYKVHDBNacgtumrwsykvhdbn", b"TGCAAKYWSRMBDHVNtgcaakywsrmbdhvn")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
U64 = np.uint64
TANDEM = 1 << 42                                                             # MM_SEED_TANDEM (mmpriv.h:20)
SEG_SHIFT = 48                                                               # MM_SEED_SEG_SHIFT (mmpriv.h:23)


def revcomp(s):
    return s.translate(COMP)[::-1]


def rng_for(name):
    return np.random.default_rng(int.from_bytes(hashlib.sha256(name.encode()).digest()[:8], "little"))


def rand_seq(rng, n):
    return ACGT[rng.integers(0, 4, int(n))].tobytes()


# ------------------------------------------------------------------------------------------------ the reference library
class SeedRef:
    """oracle/_ref/libseedref.so: built from the reference's sources where they lie, or the one that came with the tree."""

    def __init__(self):
        p = os.path.join(ROOT, "oracle", "_ref", "libseedref.so")
        if not os.path.exists(p):                                             # (build() makes it with the other reference binaries; a tree that was not built: once, here)
            subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "_ref/libseedref.so"], check=False, capture_output=True)
        if not os.path.exists(p):
            raise RuntimeError("oracle/_ref/libseedref.so is missing: the reference build (oracle/Makefile, target ref) must travel to the GPU box with the snapshot -- "
                               "without it this comparison against the reference would silently not run")
        L = self.L = C.CDLL(p)
        vp, ci = C.c_void_p, C.c_int
        L.seedref_index.restype = vp; L.seedref_index.argtypes = [ci, ci, ci, vp, vp]
        L.seedref_destroy.restype = None; L.seedref_destroy.argtypes = [vp]
        L.seedref_flag_ok.restype = ci; L.seedref_flag_ok.argtypes = [vp]
        L.seedref_get.restype = ci; L.seedref_get.argtypes = [vp, C.c_uint64, vp, ci]
        L.seedref_sketch.restype = C.c_int64; L.seedref_sketch.argtypes = [C.c_char_p, ci, ci, ci, C.c_uint32, vp, C.c_int64]
        L.seedref_frag.restype = C.c_int64; L.seedref_frag.argtypes = [vp, ci, vp, vp, ci, vp, C.c_int64, vp, vp, vp, vp, ci]
        self.buf = np.zeros((1 << 16, 2), dtype=U64); self.lbuf = np.zeros(1 << 14, dtype=np.uint32)

    def index(self, k, w, seqs, names):
        n = len(seqs)
        sa = (C.c_char_p * n)(*seqs); na = (C.c_char_p * n)(*names)
        h = self.L.seedref_index(k, w, n, sa, na)
        assert h and self.L.seedref_flag_ok(h), "mm_set_opt(\"sr\") must give MM_F_HEAP_SORT and no dust filter"
        return h

    def destroy(self, h):
        self.L.seedref_destroy(h)

    def occ(self, h, minier):
        return self.L.seedref_get(h, int(minier), None, 0)

    def sketch(self, seq, w, k, rid=0):
        """mm_sketch of one read: (n, 2) uint64."""
        cap = max(len(seq), 1)
        out = np.zeros((cap, 2), dtype=U64)
        n = self.L.seedref_sketch(seq, len(seq), w, k, rid, out.ctypes.data_as(C.c_void_p), cap)
        assert 0 <= n <= cap
        return out[:n].copy()

    def frag(self, h, seqs, max_occ):
        """Res of one fragment (its segments in mapping orientation) under the occurrence bound max_occ."""
        ns = len(seqs)
        ql = (C.c_int * ns)(*[len(s) for s in seqs]); sa = (C.c_char_p * ns)(*seqs)
        rep, nm, nmv = C.c_int(0), C.c_int(0), C.c_int(0)
        need_l = sum(len(s) for s in seqs) + 1
        if need_l > len(self.lbuf):
            self.lbuf = np.zeros(need_l * 2, dtype=np.uint32)
        while True:
            n = self.L.seedref_frag(h, ns, ql, sa, max_occ, self.buf.ctypes.data_as(C.c_void_p), len(self.buf), C.byref(rep), C.byref(nm), C.byref(nmv), self.lbuf.ctypes.data_as(C.c_void_p), len(self.lbuf))
            if n <= len(self.buf):
                break
            self.buf = np.zeros((int(n) * 2, 2), dtype=U64)
        a = self.buf[:n].copy(); lists = self.lbuf[:nm.value].copy()
        return Res(a, rep.value, lists, nmv.value)


class Res(namedtuple("Res", "anchors rep_len lists n_mv")):
    """What the reference makes of a fragment: anchors (n, 2) in its order, rep_len, the length of every list of collect_matches (lists of absent
    keys have length 0: the reference counts them in n_m, the kernels do not make a match record for them), the minimizer count."""
    @property
    def n_a(self):
        return len(self.anchors)

    @property
    def n_lists(self):                                                       # lists with at least one occurrence: what frag_nm counts
        return int((self.lists > 0).sum())

    @property
    def tied(self):
        x = self.anchors[:, 0]
        return bool(len(x) > 1 and (x[1:] == x[:-1]).any())

    @property
    def n_rev(self):
        return int((self.anchors[:, 0] >> U64(63)).sum())


_REF = []


def seedref():
    if not _REF:
        _REF.append(SeedRef())
    return _REF[0]


# ------------------------------------------------------------------------------------------------ shapes and references
Shape = namedtuple("Shape", "name n_contigs k w mid_occ max_occ full long_list")
SHAPES = {s.name: s for s in (
    Shape("c3", 3, 21, 11, 50, 200, True, False),                           # the full ladder, every directed case
    Shape("c1", 1, 21, 11, 50, 200, False, False),
    Shape("c2", 2, 21, 11, 50, 200, False, False),
    Shape("c32768", 32768, 21, 11, 50, 200, False, False),                  # rid_bits 15: the last shape with compact sort keys
    Shape("c32769", 32769, 21, 11, 50, 200, False, False),                  # rid_bits 16: k_anchor_sort<1024> and the chunked radix path
    Shape("c65536", 65536, 21, 11, 50, 200, False, False),                  # the last shape whose once-occurring minimizers sit in the table entry
    Shape("c65537", 65537, 21, 11, 50, 200, False, False),                  # ... become lists of one (the entry holds 16 contig bits)
    Shape("c3_long", 3, 21, 11, 50, 2500, False, True),                     # one family of 2100 copies: lists of 2000 and more in the re-chain pass
)}
SIZES = (0, 1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193)
GIANT = 40000
TIED_LIST_COUNTS = (2, 48, 49, 63, 64, 96, 97, 126, 127, 128, 129, 600)
TIED_LIST_LENGTHS = (16, 17, 18)
# untied fragments at the sort tables' list caps: (lists, bulk lists of LO, the anchor class they must land in)
CAP_CASES = ((512, 2, 513, 1024), (513, 2, 513, 1024), (1024, 1, 1025, 2048), (1025, 1, 1025, 2048), (1024, 25, 2049, 4096), (1025, 25, 2049, 4096),
             (1024, 70, 4097, 8192), (1025, 70, 4097, 8192), (1024, 165, 8193, 1 << 30), (1025, 165, 8193, 1 << 30))

Family = namedtuple("Family", "unit copies mixed")
Ref = namedtuple("Ref", "shape contigs names fam U u_at end_read longest")
Frag = namedtuple("Frag", "label seqs second")                              # seqs: 1 or 2 segments in mapping orientation; second: in the re-chain pass's list


def _tandem(rng, period, length):
    u = rand_seq(rng, period)
    return (u * (length // period + 2))[:length]


def build_reference(shape):
    rng = rng_for("reference " + shape.name)
    full = shape.full
    fam = {
        "LO": Family(rand_seq(rng, 7000 if full else 400), 48, True),         # the bulk of the first pass's ladder: lists of 48 < mid_occ
        "HI": Family(rand_seq(rng, 1900 if full else 150), 150, True),        # ... of the re-chain pass's: 50 <= 150 < max_occ
        "F2": Family(rand_seq(rng, 300), 2, False), "F3": Family(rand_seq(rng, 300), 3, True),
        "F16": Family(rand_seq(rng, 120), 16, False), "F17": Family(rand_seq(rng, 120), 17, False), "F18": Family(rand_seq(rng, 120), 18, False),
        "F49": Family(rand_seq(rng, 300), 49, True), "F50": Family(rand_seq(rng, 300), 50, True),
        "F199": Family(rand_seq(rng, 300), 199, True), "F200": Family(rand_seq(rng, 300), 200, True),
        "STRLO": Family(_tandem(rng, 7, 160), 1, False),                      # 20 occurrences of each of its k-mers
        "STRMID": Family(_tandem(rng, 7, 21 + 7 * 100), 1, False),            # about 100: above mid_occ, below max_occ
        "STRHI": Family(_tandem(rng, 5, 21 + 5 * 260), 1, False),             # about 260: above both
    }
    if shape.long_list:
        fam["FLONG"] = Family(rand_seq(rng, 90), 2100, True)
    n_long = min(3, shape.n_contigs); n_small = shape.n_contigs - n_long
    long_c = [[] for _ in range(n_long)]
    sp = lambda: rand_seq(rng, rng.integers(30, 51))
    blocks = []
    for name, f in fam.items():
        for j in range(f.copies):
            if name == "F2" and n_long >= 2:
                continue
            blocks.append(revcomp(f.unit) if f.mixed and j % 2 else f.unit)
    if n_long >= 2:                                                         # equal positions on different contigs: F2's two copies after 40 bases of contigs 0 and 1
        for j in range(2):
            long_c[j] += [rand_seq(rng, 40), fam["F2"].unit]
    order = rng.permutation(len(blocks))
    sizes = [sum(len(b) for b in c) for c in long_c]
    for i in order:
        j = int(np.argmin(sizes)); b = blocks[i]
        s = sp(); long_c[j] += [s, b]; sizes[j] += len(s) + len(b)
    U = rand_seq(rng, 12000)
    # the last contig ends in a read-sized piece whose last k-mer is a minimizer: an anchor on the contig's last base
    R = seedref()
    while True:
        end = rand_seq(rng, 150)
        mv = R.sketch(end, shape.w, shape.k)
        if len(mv) and int(mv[-1, 1] & U64(0xffffffff)) >> 1 == len(end) - 1:
            break
    fill = max(sizes) - sizes[-1] + 500                                      # ... and is the longest
    long_c[-1] += [sp(), rand_seq(rng, fill), sp(), U, sp(), end]
    contigs = []
    if n_small:
        lens = rng.integers(40, 65, n_small); flat = ACGT[rng.integers(0, 4, int(lens.sum()))].tobytes(); o = 0
        for L in lens:
            contigs.append(flat[o:o + int(L)]); o += int(L)
    longs = [b"".join(c) for c in long_c]
    u_at = (shape.n_contigs - 1, longs[-1].index(U))
    contigs += longs
    names = [b"s%d" % i for i in range(len(contigs))]
    lens = [len(c) for c in contigs]
    assert lens[-1] == max(lens) and lens.count(lens[-1]) == 1
    return Ref(shape, contigs, names, fam, U, u_at, end, len(contigs) - 1)


# ------------------------------------------------------------------------------------------------ fitting a fragment to a count
class Gen:
    def __init__(self, shape):
        self.shape = shape; self.ref = build_reference(shape); self.R = seedref()
        self.h = self.R.index(shape.k, shape.w, self.ref.contigs, self.ref.names)
        self.rng = rng_for("fragments " + shape.name)
        self.frags = []; self.variant = 0
        for x in self.strong_of(self.ref.U[11000:12000], 12, 0):               # one k-mer of U, twice: two lists of one anchor with equal x and nothing else
            self.single_piece = self.junk(14) + x + self.junk(15) + x + self.junk(14)
            r = self.ev((self.single_piece + self.junk(12),), False)
            if r.n_a == 2 and r.tied:
                break
        else:
            raise AssertionError("no k-mer of U is picked twice on its own")

    def close(self):
        self.R.destroy(self.h); self.h = None

    def junk(self, n):
        return rand_seq(self.rng, n)

    def ev(self, seqs, second):
        return self.R.frag(self.h, seqs, self.shape.max_occ if second else self.shape.mid_occ)

    def add(self, label, seqs, second=False):
        seqs = tuple(seqs); assert 1 <= len(seqs) <= 2
        self.frags.append(Frag(label, seqs, second))

    def fit(self, label, make, target, metric, second, t_max, check=None):
        """The fragment make(T), T the tail's length in 0 ... t_max, whose metric(Res) under the pass's bound is exactly `target`: metric does not
        decrease with T but for the last window's minimizer, so a bisection to the first T that reaches the target and a walk around it."""
        for self.variant in range(8):                                         # (a step of the tail can add two anchors at once: then the same from another place of U)
            seen = {}

            def at(T):
                if T not in seen:
                    s = make(T); seen[T] = (s, self.ev(s, second))
                return seen[T]
            lo, hi = 0, t_max
            assert metric(at(hi)[1]) >= target, "%s: %d at the longest tail, %d wanted" % (label, metric(at(hi)[1]), target)
            while lo < hi:
                mid = (lo + hi) // 2
                if metric(at(mid)[1]) >= target:
                    hi = mid
                else:
                    lo = mid + 1
            for d in range(0, 40):
                for T in (lo + d, lo - d):
                    if 0 <= T <= t_max and metric(at(T)[1]) == target and (check is None or check(at(T)[1])):
                        self.add(label, at(T)[0], second); self.variant = 0
                        return at(T)[1]
        raise AssertionError("%s: no tail length gives %d" % (label, target))

    def tail(self, T, u0):
        u0 += 173 * self.variant
        return self.ref.U[u0:u0 + T]

    def bulk_len(self, famname, want, second, pre=b"", suf=b""):
        """A prefix of the family's unit, as long as can be found, whose anchors (between `pre` and `suf`) stay at or below `want`."""
        unit = self.ref.fam[famname].unit
        lo, hi = 0, len(unit)
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if self.ev((pre + unit[:mid] + suf,), second).n_a <= want:
                lo = mid
            else:
                hi = mid - 1
        while lo > 0 and self.ev((pre + unit[:lo] + suf,), second).n_a > want:   # (the last window's minimizer comes and goes with the length)
            lo -= 1
        return lo

    def tie_piece(self, src=None, at=None, single=False):
        """A piece that holds a whole window of k-mers (40 bases: twenty k-mers), twice, 15 random bases between: one of its minimizers is picked
        in both copies whatever surrounds them, and its anchors have equal x.  single: one k-mer of U with a very small hash instead, so that the
        two copies give two lists of one anchor and nothing else."""
        if single:
            return self.single_piece
        if src is None:
            at = 11000 + 45 * (len(self.frags) % 20); d = self.ref.U[at:at + 40]
        else:
            d = self.ref.fam[src].unit[at:at + 45]
        return d + self.junk(15) + d

    # ---- the anchor cases
    def ladder(self, sizes, second):
        famname = "HI" if second else "LO"
        for n in sizes:
            for tied in ((False,) if n < 2 else (False, True)):
                label = "size %d %s pass%d" % (n, "tied" if tied else "untied", 2 if second else 1)
                if n == 0:
                    self.add(label, (self.junk(150),), second); continue
                pre = self.tie_piece(single=n < 16) + self.junk(12) if tied else b""
                c = self.ref.fam[famname].copies
                j12 = self.junk(12)
                Lb = self.bulk_len(famname, n - 2, second, pre, j12) if n >= c + 8 else 0
                bulk = pre + self.ref.fam[famname].unit[:Lb] + (j12 if Lb or pre else b"")
                u0 = 100 + 37 * (len(self.frags) % 40)
                pair = len(self.frags) % 2 == 1 and len(bulk) >= 60              # every other fragment as a pair: the bulk in mate 1, the tail in mate 2
                j25 = self.junk(25)
                make = (lambda T: (bulk, j25 + self.tail(T, u0))) if pair else (lambda T: (bulk + self.tail(T, u0),))
                r = self.fit(label, make, n, lambda r: r.n_a, second, 14 * (c + 30), check=lambda r: r.tied == tied)
                assert r.n_a == n and r.tied == tied, label

    def giant(self, second):
        famname = "HI" if second else "LO"
        for tied in (False, True):
            label = "giant %s pass%d" % ("tied" if tied else "untied", 2 if second else 1)
            pre = self.tie_piece() + self.junk(12) if tied else b""
            unit = self.ref.fam[famname].unit[:1800 if second else 5600]       # (at most 1024 lists: the run sort's table)
            r = self.ev((pre + unit,), second)
            assert r.n_a >= GIANT and r.tied == tied and r.n_lists <= 1000, (label, r.n_a, r.n_lists)
            self.add(label, (pre + unit,), second)

    def caps(self):
        lo = self.ref.fam["LO"].unit
        for n_lists, n_bulk, a_lo, a_hi in CAP_CASES:
            label = "cap %d lists, %d ... %d anchors" % (n_lists, a_lo, a_hi)
            # a prefix of LO that holds n_bulk lists
            L = 0; got = 0; j12 = self.junk(12)
            while got < n_bulk:
                L += 3; got = int((self.ev((lo[:L] + j12 + self.tail(200, 50),), False).lists >= 40).sum())
            bulk = lo[:L] + j12
            r = self.fit(label, lambda T: (bulk + self.tail(T, 50),), n_lists, lambda r: r.n_lists, False, 9000, check=lambda r: not r.tied and a_lo <= r.n_a <= a_hi)
            self.frags[-1] = self.frags[-1]._replace(second=True)              # (all lists below mid_occ: the same fragment in the re-chain pass)

    def tied_lists(self):
        for m in TIED_LIST_COUNTS:
            for second in (False, True):
                label = "tied %d lists pass%d" % (m, 2 if second else 1)
                pre = self.tie_piece(single=m == 2) + self.junk(12)
                if second and m > 2:                                         # (a piece the first pass filters: rep_len > 0, a candidate for the merges made ahead)
                    pre += self.ref.fam["HI"].unit[300:300 + 24] + self.junk(12)
                u0 = 200 + 31 * (len(self.frags) % 30)
                self.fit(label, lambda T: (pre + self.tail(T, u0),), m, lambda r: r.n_lists, second, 5000, check=lambda r: r.tied)
        for c in TIED_LIST_LENGTHS:
            for second in (False, True):
                label = "tied list length %d pass%d" % (c, 2 if second else 1)
                pre = self.tie_piece("F%d" % c, 30) + self.junk(12) + (self.ref.fam["HI"].unit[500:524] + self.junk(12) if second else b"")
                s = (pre + self.tail(60, 700),)
                r = self.ev(s, second)
                assert r.tied and (r.lists == c).sum() >= 2, label
                self.add(label, s, second)

    def long_lists(self):
        unit = self.ref.fam["FLONG"].unit
        d = unit[20:70]
        for label, s in (("long list tied", (d + self.junk(15) + d + self.junk(12) + self.tail(80, 300),)), ("long list untied", (unit[15:80] + self.junk(12) + self.tail(80, 900),)),
                         ("long list pair tied", (self.junk(30) + d, d + self.junk(40)))):
            r = self.ev(s, True)
            assert (r.lists >= 2000).any() and r.tied == ("untied" not in label), label
            self.add(label, s, True)

    def strands(self):
        f16 = self.ref.fam["F16"].unit
        fwd = f16[10:110] + self.junk(12) + self.tail(120, 1500)
        for label, s in (("strand all forward", (fwd,)), ("strand all reverse", (revcomp(fwd),)), ("strand mixed", (fwd + self.junk(12) + revcomp(self.tail(120, 1700)),)),
                         # the same reference k-mers hit in both orientations: equal (contig, position) on opposite strands, which is not a tie
                         ("strand both on one position", (self.tail(90, 2000) + self.junk(15) + revcomp(self.tail(90, 2000)),))):
            self.add(label, s, True)
        for T in range(60, 100):                                               # odd and even n_rev
            self.add("strand reverse tail %d" % T, (revcomp(self.tail(T, 2300)),), T % 2 == 0)

    def positions(self):
        ref = self.ref
        self.add("position last base of the longest contig", (ref.end_read,), True)
        self.add("position last base, reverse", (revcomp(ref.end_read),), True)
        if "F2" in ref.fam:
            self.add("position equal on two contigs", (ref.fam["F2"].unit[:150],), True)
        n = len(ref.contigs)
        for i in sorted({0, 1, n // 2, 32767, 32768, 65535, 65536, n - 4, n - 3, n - 2, n - 1}):
            if 0 <= i < n:
                c = ref.contigs[i]; s = c if len(c) <= 64 else c[len(c) // 2: len(c) // 2 + 60]
                self.add("position contig %d" % i, (s,), True)
                self.add("position contig %d reverse, pair" % i, (revcomp(s), self.junk(30)), True)
                if len(c) > 64:                                              # (a long contig's first bases are a unique spacer: once-occurring minimizers)
                    self.add("position contig %d first bases" % i, (c[:60],), True)

    # ---- the seed-lookup cases
    def strong_of(self, unit, n, margin):
        """The n minimizers of a sequence (`margin` bases from its ends) with the smallest hashes, as k-mers: picked in a read almost whatever surrounds them."""
        k = self.shape.k
        mv = self.R.sketch(unit, self.shape.w, k)
        pos = (mv[:, 1] & U64(0xffffffff)).astype(np.int64) >> 1
        keep = [(int(x >> U64(8)), int(p)) for x, p in zip(mv[:, 0], pos) if margin + k - 1 <= p < len(unit) - margin]
        keep.sort()
        return [unit[p - k + 1:p + 1] for _, p in keep[:n]]

    def strong(self, famname, n):
        return self.strong_of(self.ref.fam[famname].unit, n, 40)

    def lookup(self):
        fam = self.ref.fam
        for name in ("F49", "F50", "F199", "F200", "F2", "F3"):              # occurrence counts of bound - 1 and bound; two and three
            for st in (20, 90, 160):
                self.add("occ %s at %d" % (name, st), (self.junk(st % 7) + fam[name].unit[st:st + 110] + self.junk(10) + self.tail(40, 3000 + st),), True)
        self.add("no minimizer", (self.junk(self.shape.k - 1),), True)
        self.add("a mate without minimizers", (self.tail(150, 3300), self.junk(10)), True)
        self.add("first mate without minimizers", (self.junk(12), self.tail(150, 3500)), True)
        self.add("absent keys only", (self.junk(150), self.junk(150)), True)
        # repeat-length intervals (map.c:105-111) between two filtered minimizers X, Y that are 21 + g bases apart: touching at g = 0, one base apart at g = 1;
        # at the first and the last minimizer of the fragment; across the mate boundary
        for name in ("F200", "F50"):
            xs = self.strong(name, 6)
            for i in range(len(xs) - 1):
                X, Y = xs[i], xs[i + 1]
                for g in (0, 1, 2, 5, 30):
                    self.add("rep %s gap %d" % (name, g), (self.junk(20 + i) + X + self.junk(g) + Y + self.junk(25),), True)
                self.add("rep %s first and last" % name, (X + self.junk(40 + i) + Y,), True)
                self.add("rep %s across mates, touching" % name, (self.junk(30) + X, Y + self.junk(30 + i)), True)
                self.add("rep %s across mates, apart" % name, (self.junk(30) + X + self.junk(3), self.junk(2) + Y + self.junk(30)), True)
                self.add("rep %s whole run" % name, (fam[name].unit[30 + 10 * i:200] + self.junk(12) + self.tail(50, 3700),), True)
        # runs of equal neighbouring hashes (the tandem flag, map.c:114-115): pieces of a tandem repeat of period 7 behind 0 ... 47 random bases, so that the run
        # starts at every place of a group of four minimizers; a run that runs on into mate 2; runs whose members one or both passes filter
        for name in ("STRLO", "STRMID", "STRHI"):
            arr = fam[name].unit
            for a in range(0, 48, 3 if name != "STRLO" else 1):
                for L in ((24, 28, 31, 35, 38, 42, 49) if name == "STRLO" else (31, 42)):
                    self.add("tandem %s after %d, %d bases" % (name, a, L), (self.junk(a) + arr[:L] + self.junk(30),), (a + L) % 2 == 0)
            for ph in range(7):
                self.add("tandem %s across mates, phase %d" % (name, ph), (self.junk(20 + ph) + arr[:35], arr[ph:ph + 35] + self.junk(25)), True)
                self.add("tandem %s at both ends, phase %d" % (name, ph), (arr[ph:ph + 30] + self.junk(40) + arr[:30],), True)


_CACHE = {}


def case_set(name):
    """(Ref, [Frag], second-pass list) of a shape; generated once per process."""
    if name not in _CACHE:
        shape = SHAPES[name]
        g = Gen(shape)
        if shape.long_list:
            g.long_lists(); g.ladder((0, 1, 2, 65), False)
        else:
            sizes = SIZES if shape.full else tuple(n for n in SIZES if n <= 2049)
            g.ladder(sizes, False); g.ladder(sizes, True)
            if shape.full:
                g.giant(False); g.giant(True); g.caps()
            g.tied_lists(); g.strands(); g.positions()
            if shape.full:
                g.lookup()
        # the first pass's ladder, in the re-chain pass as well (the same anchors there: none of its lists reaches mid_occ)
        frags = [f._replace(second=True) if f.label.startswith("size ") and f.label.endswith("pass1") and i % 3 == 0 else f for i, f in enumerate(g.frags)]
        second = [i for i, f in enumerate(frags) if f.second]
        g.close()
        _CACHE[name] = (g.ref, frags, second)
    return _CACHE[name]


def upload_reads(frags):
    """(n_segs, seqs) for a batch upload: mate 2 as read."""
    n_segs, seqs = [], []
    for f in frags:
        n_segs.append(len(f.seqs)); seqs.append(f.seqs[0])
        if len(f.seqs) == 2:
            seqs.append(revcomp(f.seqs[1]))
    return n_segs, seqs


def reference_results(name):
    """[(Res of the first pass, Res of the re-chain pass or None)] per fragment, and the handle-free minimizers [(n, 2) per segment]."""
    key = ("results", name)
    if key not in _CACHE:
        ref, frags, second = case_set(name)
        R = seedref(); sh = ref.shape
        h = R.index(sh.k, sh.w, ref.contigs, ref.names)
        out = [(R.frag(h, f.seqs, sh.mid_occ), R.frag(h, f.seqs, sh.max_occ) if f.second else None) for f in frags]
        mini = [[R.sketch(s, sh.w, sh.k) for s in f.seqs] for f in frags]
        occ = {}
        for mv in mini:
            for m in mv:
                for x in m[:, 0]:
                    hsh = int(x >> U64(8))
                    if hsh not in occ:
                        occ[hsh] = R.occ(h, hsh)
        R.destroy(h)
        _CACHE[key] = (out, mini, occ)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ sketch cases
SKETCH_SETS = ((21, 11), (21, 10), (15, 5), (19, 1), (22, 32), (25, 11), (26, 32), (28, 12))
SKETCH_BATCHES = (1, 63, 64, 65)


def sketch_reads(k, w):
    """The reads of one option set (k, w), deterministic."""
    key = ("sketch", k, w)
    if key in _CACHE:
        return _CACHE[key]
    rng = rng_for("sketch %d %d" % (k, w))
    lens = sorted({0, 1, k - 1, k, k + w - 2, k + w - 1, k + w, 7, 8, 9, 15, 16, 17, 150, 250})
    out = []
    for L in lens:
        out.append(("random %d" % L, rand_seq(rng, L)))
    if (k, w) == (25, 11):                                                   # the packed entry's position limit: from 8192 bases the whole batch takes the wide form
        out += [("random 8191", rand_seq(rng, 8191)), ("random 8192", rand_seq(rng, 8192))]
    for L in (k + w + 3, 150, 250):
        for nm, unit in (("homopolymer", b"A"), ("AC", b"AC"), ("AT", b"AT"), ("ACGT", b"ACGT"), ("ACG", b"ACG"), ("period 7", rand_seq(rng, 7)), ("period 11", rand_seq(rng, 11))):
            out.append(("%s %d" % (nm, L), (unit * (L // len(unit) + 1))[:L]))
        half = rand_seq(rng, L // 2)
        out.append(("inverted repeat %d" % L, half + revcomp(half)))                                   # palindromic k-mers at its centre when k is even
        out.append(("all N %d" % L, b"N" * L))
        out.append(("lower case %d" % L, rand_seq(rng, L).lower()))
        s = bytearray(rand_seq(rng, L))
        for p in rng.integers(0, L, 6):
            s[int(p)] = b"RYKMSWBDHVUn"[int(p) % 12]
        out.append(("IUPAC %d" % L, bytes(s)))
    for at in sorted({0, 1, 7, 8, 9, 15, 16, 17, k - 1, k, k + 1, k + w - 2, k + w - 1, k + w, 100, 149}):   # around 8 i, around the window's first and last slot
        for run in (1, 2, 8, k):
            s = bytearray(rand_seq(rng, 150))
            s[at:at + run] = b"N" * len(s[at:at + run])
            out.append(("N run of %d at %d" % (run, at), bytes(s)))
    _CACHE[key] = out
    return out


# ------------------------------------------------------------------------------------------------ the project's own CPU oracle
class _OIdx(C.Structure):                                                     # oidx_t (oracle/al_oracle.h)
    _fields_ = [("k", C.c_int), ("w", C.c_int), ("n_seq", C.c_uint32), ("seq", C.c_void_p), ("S", C.c_void_p), ("tot_len", C.c_uint64), ("n_keys", C.c_uint64),
                ("keys", C.POINTER(C.c_uint64)), ("vals", C.POINTER(C.c_uint64)), ("tab_mask", C.c_uint64), ("pos", C.POINTER(C.c_uint64)), ("n_pos", C.c_uint64)]


class Oracle:
    """o_sketch, oidx_build and o_collect_seeds of oracle/libal_oracle.so."""

    def __init__(self):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libal_oracle.so"], check=True, capture_output=True)
        L = self.L = C.CDLL(os.path.join(ROOT, "oracle", "libal_oracle.so"))
        vp, ci = C.c_void_p, C.c_int
        L.oidx_build.restype = C.POINTER(_OIdx); L.oidx_build.argtypes = [ci, ci, ci, vp, vp]
        L.oidx_destroy.restype = None; L.oidx_destroy.argtypes = [C.POINTER(_OIdx)]
        L.o_sketch.restype = None; L.o_sketch.argtypes = [C.c_char_p, ci, ci, ci, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.o_collect_seeds.restype = vp; L.o_collect_seeds.argtypes = [C.POINTER(_OIdx), ci, vp, C.c_size_t, ci, C.POINTER(C.c_int64), C.POINTER(ci)]
        self.free = C.CDLL(None).free; self.free.restype = None; self.free.argtypes = [vp]

    def index(self, k, w, seqs, names):
        n = len(seqs)
        return self.L.oidx_build(k, w, n, (C.c_char_p * n)(*names), (C.c_char_p * n)(*seqs))

    def destroy(self, h):
        self.L.oidx_destroy(h)

    def positions(self, h):
        return np.ctypeslib.as_array(h.contents.pos, (int(h.contents.n_pos),)).copy()

    def positions_by_key(self, h):
        """The occurrence array with the lists in ascending order of their keys (the hash table's slots hold key + 1 and offset << 32 | count)."""
        n = int(h.contents.tab_mask) + 1
        keys = np.ctypeslib.as_array(h.contents.keys, (n,)); vals = np.ctypeslib.as_array(h.contents.vals, (n,))
        used = np.nonzero(keys)[0]
        used = used[np.argsort(keys[used], kind="stable")]
        pos = self.positions(h)
        off = (vals[used] >> U64(32)).astype(np.int64); cnt = (vals[used] & U64(0xffffffff)).astype(np.int64)
        idx = np.repeat(off - np.concatenate(([0], np.cumsum(cnt)[:-1])), cnt) + np.arange(int(cnt.sum()))
        return pos[idx], len(used)

    def sketch(self, seq, w, k, rid=0):
        a = C.c_void_p(None); n = C.c_size_t(0); m = C.c_size_t(0)
        if len(seq):
            self.L.o_sketch(seq, len(seq), w, k, rid, C.byref(a), C.byref(n), C.byref(m))
        out = np.ctypeslib.as_array(C.cast(a, C.POINTER(C.c_uint64)), (n.value * 2,)).reshape(-1, 2).copy() if n.value else np.zeros((0, 2), dtype=U64)
        if a.value:
            self.free(a)
        return out

    def frag(self, h, seqs, max_occ):
        """(anchors, rep_len) of o_collect_seeds on the fragment's minimizers, collected as collect_minimizers does (map.c:64-77)."""
        k, w = h.contents.k, h.contents.w
        mv = []; tot = 0
        for i, s in enumerate(seqs):
            m = self.sketch(s, w, k, i); m[:, 1] += U64(tot << 1); mv.append(m); tot += len(s)
        mv = np.ascontiguousarray(np.concatenate(mv))
        na = C.c_int64(0); rep = C.c_int(0)
        p = self.L.o_collect_seeds(h, max_occ, mv.ctypes.data_as(C.c_void_p), len(mv), tot, C.byref(na), C.byref(rep))
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), (na.value * 2,)).reshape(-1, 2).copy() if na.value else np.zeros((0, 2), dtype=U64)
        self.free(p)
        return a, rep.value

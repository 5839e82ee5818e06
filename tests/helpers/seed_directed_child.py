"""One configuration of tests/test_gpu_seed_directed.py, in a process of its own (the environment switches are read once per process): a case set of
tests/seed_cases.py through the seed stage's own code (al_dbg_seed: sketch, seed lookup, anchor collection, sorts and merges as a batch run launches
them, without the chaining) against the reference library, read by read and fragment by fragment.

usage: seed_directed_child.py <shape>            the shape's fragments, first pass and re-chain pass   (the environment carries AL_TEST_SORT_BLK, AL_BIG_MERGE, ...)
       seed_directed_child.py sketch <k> <w>     the sketch reads of one option set, first pass on a tiny index
Prints one JSON line: generated, compared, the first mismatches in full, per pass the counts that say which kernels did the work and the counts
this file expects from the reference's results, and the seconds the steps took."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import seed_cases as K  # noqa: E402

# The sort kernels' tables, stated once: kernel -> (most anchors, most occurrence lists) it orders itself; a fragment beyond either is flagged for the
# exact heap merge, like one with equal x.  (The dispatch never hands a kernel more anchors than it holds; list counts it does not look at.)
CAPS = {"small": (64, None), "reg_2_1_128": (128, 128), "reg_4_1_256": (256, 256), "reg_8_1_512": (512, 512), "reg_16_1_512": (1024, 512), "reg_8_4_1024": (2048, 1024),
        "reg_16_4_1024": (4096, 1024), "reg_16_8_1024": (8192, 1024), "sort1024": (1024, 512), "merge": (None, 1024), "radix": (None, None)}


def anchor_y(y):
    """The reference's y of an anchor from the kernels': identical -- span << 32 | query position, the segment from bit 48 and MM_SEED_TANDEM (bit 42) are the
    reference's own bits, and the kernels keep no bit of their own in an anchor."""
    return y


class Dispatch:
    """Which sort kernel run_seed_chain gives a fragment of n anchors to: the size classes of chain_plan under the switches in force."""

    def __init__(self, n_contigs, max_len):
        e = os.environ
        self.t_blk = min(max(int(e.get("AL_TEST_SORT_BLK", 1025)), 65), 1025)
        self.t_big = min(max(int(e.get("AL_TEST_SORT_BIG", 8193)), self.t_blk), 8193)
        self.rid_bits = 1
        while (1 << self.rid_bits) < n_contigs:
            self.rid_bits += 1
        self.pos_bits = 1
        while self.pos_bits < 31 and (1 << self.pos_bits) < max_len:
            self.pos_bits += 1
        self.compact = 33 + self.rid_bits + 16 <= 64
        if not self.compact:
            self.t_big = self.t_blk
        self.rank_bits = 64 - 16 - 1 - self.rid_bits - self.pos_bits
        self.big_merge = int(e.get("AL_BIG_MERGE", 1))
        self.chunk = min(1 << min(self.rank_bits, 31), int(e.get("AL_TEST_BIG_CHUNK", 1 << 31)))
        run = e.get("AL_TEST_RUN", "8192,2048").split(",")
        self.run_len, self.tile = int(run[0]), int(run[1])

    def kernel(self, n, first):
        t_blk, t_big = self.t_blk, self.t_big
        if n < 65:
            return "small"
        if not self.compact:
            return "sort1024" if n < t_blk else "radix"
        for name, bound in (("reg_2_1_128", min(129, t_blk)), ("reg_4_1_256", min(257, t_blk)), ("reg_8_1_512", min(513, t_blk)), ("reg_16_1_512", t_blk),
                            ("reg_8_4_1024", min(max(t_blk, 2049), t_big)), ("reg_16_4_1024", min(max(t_blk, 4097), t_big)), ("reg_16_8_1024", t_big)):
            if n < bound:
                return name
        return "merge" if self.big_merge == 1 or (self.big_merge == 2 and not first) else "radix"

    def expected(self, sizes, first):
        """The tap's host-side counts for a pass over fragments of these anchor counts."""
        c = {k: 0 for k in CAPS}
        for n in sizes:
            c[self.kernel(n, first)] += 1
        out = {k: v for k, v in c.items() if k not in ("merge", "radix")}
        big = [n for n in sizes if self.kernel(n, first) in ("merge", "radix")]
        out["merge_frags"] = c["merge"]; out["radix_frags"] = c["radix"]
        out["merge_tiles"] = sum((n + self.tile - 1) // self.tile for n in big) if c["merge"] else 0
        p = 0
        if c["merge"]:
            p = 1
            while (self.run_len << p) < max(big):
                p += 1
        out["merge_passes"] = p
        out["radix_chunks"] = (c["radix"] + self.chunk - 1) // self.chunk
        out.update(compact=int(self.compact), rid_bits=self.rid_bits, pos_bits=self.pos_bits, rank_bits=self.rank_bits, nl=len(sizes), flag_all=0)
        return out


def heap_form(n, n_m, n_frag):
    """Which merge kernel run_seed_chain leaves a flagged fragment of n anchors in n_m lists to, in a batch of n_frag fragments."""
    e = os.environ
    if e.get("AL_HEAP_OLD") != "1":                                         # the heap in the lanes of a wavefront up to 63 / 126 lists, the serial form in HBM scratch above
        return "heap_lanes1" if n_m <= 63 else "heap_lanes2" if n_m <= 126 else "heap_serial0"
    wave = int(e.get("AL_TEST_HEAP_WAVE", -1))
    if wave < 0:
        wave = 16384 if n_frag >= 400000 else 8192
    if n >= wave and n_m <= 128:                                            # a wavefront per fragment; the serial forms by list count: LDS heaps of 48 and 96 entries, HBM scratch above
        return "heap_wave"
    return "heap_serial48" if n_m <= 48 else "heap_serial96" if n_m <= 96 else "heap_serial0"


HEAP_FORMS = ("heap_lanes2", "heap_lanes1", "heap_serial0", "heap_wave", "heap_serial48", "heap_serial96")


def compare_pass(bad, label, frags, ids, want, got, disp, first):
    """One pass: the fragments `ids` against the reference's results want[i]; returns the summary the test asserts on."""
    na, nm, rep, a_off, flags, anchors, cnt = (got[k] for k in ("frag_na", "frag_nm", "frag_rep", "a_off", "flags", "anchors", "counts"))
    n_cmp = 0; flag1 = flag2 = 0; tied_by_lists = [0, 0, 0]; flagged_untied = 0
    forms = {k: 0 for k in HEAP_FORMS}; flag1_over_126 = flag1_to_128 = 0
    for i in ids:
        r = want[i]; f = frags[i]; what = None
        o = int(a_off[i]); n = int(na[i])
        kern = disp.kernel(r.n_a, first)
        over = CAPS[kern][1] is not None and r.n_lists > CAPS[kern][1]
        if n != r.n_a or int(rep[i]) != r.rep_len or int(nm[i]) != r.n_lists:
            what = "n_a %d, rep_len %d, lists %d; reference %d, %d, %d" % (n, int(rep[i]), int(nm[i]), r.n_a, r.rep_len, r.n_lists)
        elif o + n > len(anchors):
            what = "anchors past the end of the array"
        else:
            a = anchors[o:o + n]
            if not np.array_equal(a[:, 0], r.anchors[:, 0]) or not np.array_equal(anchor_y(a[:, 1]), r.anchors[:, 1]):
                j = int(np.argmax((a != r.anchors).any(axis=1)))
                what = "anchor %d of %d: (%x, %x), reference (%x, %x)" % (j, n, int(a[j, 0]), int(a[j, 1]), int(r.anchors[j, 0]), int(r.anchors[j, 1]))
            elif (flags[i] != 0) != (r.tied or over):
                what = "flag word %d, but tied %s, %d lists in %s" % (int(flags[i]), r.tied, r.n_lists, kern)
            elif flags[i] > (1 if first else 2):
                what = "flag word %d" % int(flags[i])
        if what:
            bad.append("%s, %s (%s): %s" % (label, f.label, kern, what))
        n_cmp += 1
        flag1 += int(flags[i] == 1); flag2 += int(flags[i] == 2)
        if flags[i] == 1 and r.n_a > 0:
            forms[heap_form(r.n_a, r.n_lists, len(frags))] += 1
            flag1_over_126 += int(r.n_lists > 126); flag1_to_128 += int(r.n_lists <= 128)
        if r.tied:
            tied_by_lists[0 if r.n_lists <= 63 else 1 if r.n_lists <= 126 else 2] += 1
        flagged_untied += int(over and not r.tied)
    exp = disp.expected([want[i].n_a for i in ids], first)
    for k, v in exp.items():
        if cnt[k] != v:
            bad.append("%s: count %s is %d, %d expected from the reference's anchor counts" % (label, k, cnt[k], v))
    for k, v in forms.items():
        if cnt[k] != v:
            bad.append("%s: %s merged %d fragments, %d expected from the flag words and the reference's list counts" % (label, k, cnt[k], v))
    if cnt["heap_merges"] != flag1 or cnt["flagged"] != flag1 or cnt["spec_taken"] != flag2:
        bad.append("%s: %d heap merges, %d on the merge kernels' list, %d merges taken; flag words: %d of 1, %d of 2" % (label, cnt["heap_merges"], cnt["flagged"], cnt["spec_taken"], flag1, flag2))
    return {"compared": n_cmp, "counts": cnt, "flag1": flag1, "flag2": flag2, "tied_1_63": tied_by_lists[0], "tied_64_126": tied_by_lists[1], "tied_over_126": tied_by_lists[2],
            "flagged_untied": flagged_untied, "flag1_over_126": flag1_over_126, "flag1_to_128": flag1_to_128, "anchors": int(sum(want[i].n_a for i in ids))}


def compare_minimizers(bad, ctx, n_reads, want, labels):
    cnt = ctx.tap("mini_cnt", np.uint32, n_reads); off = ctx.tap("mini_off", np.uint64, n_reads + 1)
    mini = ctx.tap("mini", np.uint64, int(off[-1]) * 2).reshape(-1, 2)
    for r in range(n_reads):
        got = mini[int(off[r]): int(off[r]) + int(cnt[r])]
        if int(cnt[r]) != len(want[r]) or not np.array_equal(got, want[r]):
            bad.append("minimizers of read %d (%s): %d, reference %d" % (r, labels[r], int(cnt[r]), len(want[r])))
    return n_reads


def run_shape(name):
    import airlift_amd as A
    t0 = time.time()
    ref, frags, second = K.case_set(name)
    res, mini, occ = K.reference_results(name)
    sh = ref.shape
    t_gen = time.time() - t0; t0 = time.time()
    idx = A.Index(seqs=ref.contigs, names=ref.names, k=sh.k, w=sh.w)
    idx.mo.mid_occ, idx.mo.max_occ = sh.mid_occ, sh.max_occ               # (before the context is made: it takes a copy)
    ctx = A.Context(idx)
    t_idx = time.time() - t0; t0 = time.time()
    n_segs, seqs = K.upload_reads(frags)
    ctx.upload(n_segs, seqs, [b"f%d" % i for i, f in enumerate(frags) for _ in f.seqs])
    p1, p2 = ctx.seed(np.array(second, dtype=np.uint32))
    t_gpu = time.time() - t0
    bad = []
    disp = Dispatch(sh.n_contigs, max(len(c) for c in ref.contigs))
    want_mini = [m for mv in mini for m in mv]; labels = [f.label for f in frags for _ in f.seqs]
    n_reads = compare_minimizers(bad, ctx, len(seqs), want_mini, labels)
    s1 = compare_pass(bad, "first pass", frags, range(len(frags)), [r[0] for r in res], p1, disp, True)
    # the re-chain pass: its fragments behind the first pass's anchors and one slot per fragment, in ascending order and back to back; the others untouched
    base = int(p1["a_off"][len(frags)]) + len(frags); o = base
    for i in second:
        if int(p2["a_off"][i]) != o:
            bad.append("re-chain pass: fragment %d starts at %d, %d expected" % (i, int(p2["a_off"][i]), o)); break
        o += res[i][1].n_a
    s2 = compare_pass(bad, "re-chain pass", frags, second, [r[1] for r in res], p2, disp, False)
    for i in (i for i in range(len(frags)) if not frags[i].second):
        o, n = int(p1["a_off"][i]), int(p1["frag_na"][i])
        if int(p2["a_off"][i]) != o or int(p2["frag_na"][i]) != n or int(p2["frag_rep"][i]) != int(p1["frag_rep"][i]) or not np.array_equal(p2["anchors"][o:o + n], p1["anchors"][o:o + n]):
            bad.append("re-chain pass changed fragment %d, which is not on its list (%s)" % (i, frags[i].label))
    ctx.close(); idx.close()
    print(json.dumps({"generated": len(frags), "compared": s1["compared"], "generated2": len(second), "compared2": s2["compared"], "reads": len(seqs), "reads_compared": n_reads,
                      "n_mismatch": len(bad), "mismatches": bad[:6], "pass1": s1, "pass2": s2, "n_contigs": sh.n_contigs,
                      "seconds": {"generate": round(t_gen, 2), "index": round(t_idx, 2), "gpu": round(t_gpu, 2), "compare": round(time.time() - t0 - t_gpu, 2)}}))


def run_sketch(k, w):
    import airlift_amd as A
    t0 = time.time()
    R = K.seedref()
    reads = K.sketch_reads(k, w)
    want = [R.sketch(s, w, k) for _, s in reads]
    rng = K.rng_for("sketch index")
    idx = A.Index(seqs=[K.rand_seq(rng, 3000)], names=[b"chr"], k=k, w=w)
    ctx = A.Context(idx)
    bad = []; n = 0; batches = []; forms = []
    longest = max(len(s) for _, s in reads)
    sel = [list(range(len(reads)))]
    if longest >= 8192:                                                     # ... and the same reads without the one that switches the batch to the wide form
        sel.append([i for i, (_, s) in enumerate(reads) if len(s) < 8192])
    for nb in K.SKETCH_BATCHES:                                               # 1, 63, 64, 65 reads: the last wavefront full, one lane short, one lane over
        sel.append([(7 * j + nb) % len(reads) for j in range(nb)])
    for ids in sel:
        ctx.upload([1] * len(ids), [reads[i][1] for i in ids], [b"r%d" % i for i in ids])
        forms.append(ctx.seed()[0]["counts"]["sketch_form"])
        n += compare_minimizers(bad, ctx, len(ids), [want[i] for i in ids], [reads[i][0] for i in ids])
        batches.append(len(ids))
    ctx.close(); idx.close()
    print(json.dumps({"generated": sum(batches), "compared": n, "n_mismatch": len(bad), "mismatches": bad[:6], "batches": batches, "sketch_forms": forms, "with_8192": [int(any(len(reads[i][1]) >= 8192 for i in ids)) for ids in sel], "minimizers": int(sum(len(x) for x in want)),
                      "longest": longest, "seconds": round(time.time() - t0, 2)}))


if __name__ == "__main__":
    if sys.argv[1] == "sketch":
        run_sketch(int(sys.argv[2]), int(sys.argv[3]))
    else:
        run_shape(sys.argv[1])

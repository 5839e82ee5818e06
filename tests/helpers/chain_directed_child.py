"""One configuration of tests/test_gpu_chain_directed.py, in a process of its own (the environment switches are read once per process): the
directed anchor sets of tests/chain_cases.py through the chain stage's own code (al_dbg_chain) against mm_chain_dp, fragment by fragment.

usage: chain_directed_child.py <option set> [<file for all mismatches>]     (the environment carries AL_TEST_TILE_ALL, AL_CHAIN_COOP, AL_DBG, ...)
The fragments go in batches by read lengths, so that each gets the max_dist_x / max_dist_y of its own qlen_sum.  Prints one JSON line:
generated, compared, the first mismatches in full, and the counts that say which kernels did the work, summed over the batches."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import chain_cases as K  # noqa: E402

LO32 = np.uint64(0xffffffff)


def compare(optname, f, want, nu, uu, oo, ch):
    """None, or what differs between the stage's result for fragment f (its chain list uu / oo, its range ch of chained[]) and the reference's."""
    wu, wch = want
    na = len(f.anchors)
    cnt = (uu & LO32).astype(np.int64)
    if (oo.astype(np.int64) + cnt > na).any():
        return "a chain runs past the fragment's range: uo %s, counts %s, %d anchors" % (oo.tolist()[:8], cnt.tolist()[:8], na)
    got = np.concatenate([ch[int(o):int(o) + int(n)] for o, n in zip(oo, cnt)]) if nu else np.zeros((0, 2), dtype=np.uint64)
    if nu == len(wu) and np.array_equal(uu, wu) and np.array_equal(got, wch):
        return None
    what = "n_u %d, reference %d" % (nu, len(wu)) if nu != len(wu) else "u[] (score << 32 | count)" if not np.array_equal(uu, wu) else "the chained anchors"
    return "%s: %s\n  stage     %s\n  reference %s" % (what, K.describe(optname, f), K.chains_str(uu, got) if len(got) == cnt.sum() else uu.tolist()[:8], K.chains_str(wu, wch))


def main():
    optname = sys.argv[1]
    import airlift_amd as A
    o = K.OPTION_SETS[optname]
    fr = K.cases(optname)
    ref = K.ref_chain()
    want = [ref(o, f) for f in fr]
    groups = {}                                                             # (k, read lengths) -> fragments, in the list's order
    for i, f in enumerate(fr):
        groups.setdefault((f.k or o.k, f.qlens), []).append(i)
    rng = np.random.default_rng(3)
    refseq = bytes(b"ACGT"[c] for c in rng.integers(0, 4, 4000))
    ctxs = {}

    def context(k):
        """An index of that k (the chain kernels take the span and lmin from it) with the option set in force, and its context."""
        if k not in ctxs:
            idx = A.Index(seqs=[refseq], names=[b"chr"], k=k, w=11)
            m = idx.mo
            m.bw, m.max_gap, m.max_gap_ref, m.max_frag_len, m.min_cnt, m.min_chain_score, m.max_chain_skip, m.max_chain_iter = o[:8]
            ctxs[k] = (idx, A.Context(idx))
        return ctxs[k][1]
    bad = []; compared = 0; total = {}; tied = 0; flagged = 0; empty_between = 0
    # fragments with tied chain starts among more than 64 chains go to the chain-order kernels: a block of sixteen wavefronts from AL_ORDER_BLOCK chains on
    block = int(os.environ.get("AL_ORDER_BLOCK", "128")); order_block = order_wave = 0
    for (k_idx, qlens), ids in groups.items():
        n = len(ids); ctx = context(k_idx)
        ctx.upload([len(qlens)] * n, [b"A" * L for _ in ids for L in qlens], [b"f%d" % i for i in ids for _ in qlens])
        a_off = np.zeros(n + 1, dtype=np.uint64)
        a_off[1:] = np.cumsum([len(fr[i].anchors) for i in ids])
        anchors = np.concatenate([fr[i].anchors for i in ids])
        tie = np.array([1 if fr[i].tie else 0 for i in ids], dtype=np.uint32)
        nu, u, uo, chained, cnt = ctx.chain(anchors, a_off, tie)
        for k, v in cnt.items():
            total[k] = (total.get(k, 0) + v) if k not in ("lds_ok", "tiles_ok", "lmin") else min(total.get(k, v), v)
        total["lds_ok_any"] = max(total.get("lds_ok_any", 0), cnt["lds_ok"])
        for j, i in enumerate(ids):
            base = int(a_off[j]) + j; k = int(nu[j])
            if k > len(fr[i].anchors):
                bad.append("n_u %d of a fragment of %d anchors: %s" % (k, len(fr[i].anchors), K.describe(optname, fr[i])))
            else:
                r = compare(optname, fr[i], want[i], k, u[base:base + k], uo[base:base + k], chained[int(a_off[j]):int(a_off[j + 1])])
                if r:
                    bad.append(r)
            compared += 1
            tied += K.tied_starts(*want[i]); flagged += int(tie[j])
            if len(want[i][0]) > 64 and K.tied_starts(*want[i]):
                order_block += len(want[i][0]) >= block; order_wave += len(want[i][0]) < block
            if 0 < j < n - 1 and len(want[i][0]) == 0 and len(want[ids[j - 1]][0]) and len(want[ids[j + 1]][0]):
                empty_between += 1
    for idx, ctx in ctxs.values():
        ctx.close(); idx.close()
    if len(sys.argv) > 2:                                                   # (by hand: every mismatch, in full)
        open(sys.argv[2], "w").write("\n".join(bad))
    print(json.dumps({"generated": len(fr), "compared": compared, "n_mismatch": len(bad), "mismatches": bad[:4], "counts": total, "batches": len(groups),
                      "tied_starts": tied, "order_block_frags": int(order_block), "order_wave_frags": int(order_wave), "flagged": flagged, "empty_between_kept": empty_between, "anchors": int(sum(len(f.anchors) for f in fr)),
                      "chains_max": max(len(w[0]) for w in want), "over_64_anchors": sum(1 for f in fr if len(f.anchors) > 64)}))


if __name__ == "__main__":
    main()

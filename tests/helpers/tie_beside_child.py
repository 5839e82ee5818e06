"""One process of tests/test_gpu_tie_beside.py::test_both_rounds_reach_every_shared_structure: ONE al_dbg_chain batch in which the flagged fragments
(the second round) and the unflagged ones (the first) hold the same work -- every fragment of tests/chain_cases.py's size, dense and order families
of up to 2000 anchors, once with the tie flag and once without.  The flag only decides the round: the anchors are the caller's, already in order.

usage: tie_beside_child.py <runs>      (the environment carries AL_TRACE and the switches)
Prints one JSON line: per run a digest of every fragment's result (n_u, u[], uo[], the chains' anchors), and what the two copies of a fragment gave."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import chain_cases as K  # noqa: E402

LO32 = np.uint64(0xffffffff)


def batch():
    o = K.SR
    fr = [f for f in K.sizes(o) + K.dense(o) + K.order(o) if len(f.anchors) <= 2000 and sum(f.qlens) <= 4095]
    return fr + fr, np.array([0] * len(fr) + [1] * len(fr), dtype=np.uint32)


def fragment_digests(fr, a_off, nu, u, uo, ch):
    out, free = [], []                                                        # free: without uo[] (where a kernel puts a chain inside the fragment's range is its own choice)
    for j, f in enumerate(fr):
        base = int(a_off[j]) + j; k = int(nu[j])
        uu = u[base:base + k]; oo = uo[base:base + k].astype(np.int64); cnt = (uu & LO32).astype(np.int64)
        assert k <= len(f.anchors) and (oo + cnt <= len(f.anchors)).all(), f.label
        rng = ch[int(a_off[j]):int(a_off[j + 1])]
        h = hashlib.sha256(np.uint32(k).tobytes() + uu.tobytes() + uo[base:base + k].tobytes()); g = hashlib.sha256(np.uint32(k).tobytes() + uu.tobytes())
        for o_, n_ in zip(oo, cnt):
            h.update(rng[int(o_):int(o_) + int(n_)].tobytes()); g.update(rng[int(o_):int(o_) + int(n_)].tobytes())
        out.append(h.hexdigest()); free.append(g.hexdigest())
    return out, free


def main():
    runs = int(sys.argv[1])
    import airlift_amd as A
    fr, tie = batch()
    o = K.SR
    rng = np.random.default_rng(3)
    idx = A.Index(seqs=[bytes(b"ACGT"[c] for c in rng.integers(0, 4, 4000))], names=[b"chr"], k=o.k, w=11)
    m = idx.mo
    m.bw, m.max_gap, m.max_gap_ref, m.max_frag_len, m.min_cnt, m.min_chain_score, m.max_chain_skip, m.max_chain_iter = o[:8]
    ctx = A.Context(idx)
    n = len(fr)
    ctx.upload([len(f.qlens) for f in fr], [b"A" * L for f in fr for L in f.qlens], [b"f%d" % i for i, f in enumerate(fr) for _ in f.qlens])
    a_off = np.zeros(n + 1, dtype=np.uint64); a_off[1:] = np.cumsum([len(f.anchors) for f in fr])
    anchors = np.concatenate([f.anchors for f in fr])
    digests, counts, halves_equal = [], [], []
    for _ in range(runs):
        nu, u, uo, ch, cnt = ctx.chain(anchors, a_off, tie)
        d, g = fragment_digests(fr, a_off, nu, u, uo, ch)
        digests.append(hashlib.sha256("".join(d).encode()).hexdigest()); counts.append(cnt)
        halves_equal.append(g[:n // 2] == g[n // 2:])                        # a fragment's chains do not depend on the round that made them
    ctx.close(); idx.close()
    print(json.dumps({"fragments": n, "flagged": int(tie.sum()), "anchors_max": max(len(f.anchors) for f in fr), "digests": digests, "counts": counts, "halves_equal": halves_equal}))


if __name__ == "__main__":
    main()

"""One configuration of tests/test_gpu_align_directed.py, in a process of its own (the environment switches are read once per process): the directed
fragments of tests/align_cases.py through the extension stage (al_dbg_align: al_run_align_stage to its end, inside the arena-overflow loop) against the
reference's functions (oracle/_ref/libalignref.so), fragment by fragment, mate by mate, record by record and CIGAR word by CIGAR word.

usage: align_directed_child.py <option set> <cases|long|arena> [<file for all mismatches>]     (the environment carries AL_DBG, AL_PREP_HEAVY, ...)
The fragments go in batches by their longest read: a batch's longest read picks the LDS tile.  The reads are uploaded in sequencing orientation (mate 2
of a pair reverse-complemented back) and the records fetched as al_batch_fetch returns them, so the reference's records of mate 2 are flipped the
way map.c:486-497 flips them.  Prints one JSON line: generated, compared, the first mismatches in full, and the tap's counts summed over the batches."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import align_cases as K  # noqa: E402

COMPARED = tuple(n for n in K.FIELDS if n not in ("has_p", "trans_strand"))    # has_p is n_cigar > 0 in a fetched record; trans_strand is 0 under sr (the CPU test asserts it) and no field of al_reg1_t
SUMMED = ("n_early", "n_slow", "solo_early", "solo_slow", "mono_all", "long_mode", "wave_prep", "wave_finish", "closed_form", "n_jobs", "limit", "log_miss", "arena_overflow", "reruns", "records",
          "dp_lane16", "dp_lane32", "dp_lane64", "dp_g1", "dp_g2", "dp_g4", "dp_g8", "dp_g22", "dp_g32", "dp_lds")


def main():
    optname, which = sys.argv[1], sys.argv[2]
    import airlift_amd as A
    o = K.OPTION_SETS[optname]
    t0 = time.time()
    fr = {"cases": K.cases, "long": K.long_cases, "arena": K.arena_cases}[which](optname)
    _, want = K.reference(optname, which)
    t_gen = time.time() - t0
    groups = {}
    for i, f in enumerate(fr):
        groups.setdefault(max(f.qlens), []).append(i)
    idx = A.Index(seqs=list(K.CONTIGS), names=list(K.NAMES), k=o.k, w=K.W)
    m = idx.mo
    for n in K.IOPT[1:] + K.FOPT:
        setattr(m, n, getattr(o, n))
    ctx = A.Context(idx)
    bad = []; compared = 0; total = {k: 0 for k in SUMMED}; tiles = {}; t_gpu = 0.0; tile_wrong = []
    for L, ids in sorted(groups.items()):
        n = len(ids); ns = [len(fr[i].qlens) for i in ids]
        seqs = [s if j == 0 else K.revcomp(s) for i in ids for j, s in enumerate(fr[i].seqs)]
        ctx.upload(ns, seqs, [K.frag_name(i) for i in ids for _ in fr[i].qlens])
        a_off = np.zeros(n + 1, dtype=np.uint64); a_off[1:] = np.cumsum([len(fr[i].anchors) for i in ids])
        tot = int(a_off[-1])
        chained = np.concatenate([fr[i].anchors for i in ids]) if tot else np.zeros((0, 2), dtype=np.uint64)
        nu = np.array([len(fr[i].u) for i in ids], dtype=np.uint32); u = np.zeros(tot + n + 1, dtype=np.uint64); uo = np.zeros(tot + n + 1, dtype=np.uint32)
        for j, i in enumerate(ids):
            base = int(a_off[j]) + j; k = len(fr[i].u)
            u[base:base + k] = fr[i].u
            uo[base:base + k] = np.concatenate([[0], np.cumsum((fr[i].u & np.uint64(0xffffffff)).astype(np.int64))[:-1]]) if k else []
        rep = np.array([fr[i].rep_len for i in ids], dtype=np.int32)
        t1 = time.time()
        c = ctx.align(nu, u, uo, chained, a_off, rep)
        n_regs, regs, _ = ctx.fetch()
        t_gpu += time.time() - t1
        for k_ in SUMMED:
            total[k_] += c[k_]
        tiles[str(c["tmax"])] = tiles.get(str(c["tmax"]), 0) + 1
        if c["tmax"] != K.tile_of(o, L) or bool(c["long_mode"]) != (K.tile_of(o, L) == 0):
            tile_wrong.append((L, c["tmax"]))
        rd = 0
        for i in ids:
            f, w = fr[i], want[i]; why = None
            for s in range(len(f.qlens)):
                cnt = int(n_regs[rd + s]); wh = w.hits[s]
                if cnt != len(wh):
                    why = "mate %d has %d records, the reference %d" % (s, cnt, len(wh)); break
                for h in range(cnt):
                    g = regs[rd + s][h]; e = dict(zip(K.FIELDS, wh[h].tolist()))
                    if s == 1:                                                 # (map.c:486-497: back to the read as it was sequenced)
                        e["qs"], e["qe"], e["rev"] = f.qlens[1] - e["qe"], f.qlens[1] - e["qs"], 1 - e["rev"]
                    for name in COMPARED:
                        v = int(getattr(g, name))
                        if name == "hash":
                            v = v - (1 << 32) if v >= 1 << 31 else v
                        if v != e[name]:
                            why = "mate %d record %d: %s is %d, the reference's %d\n  stage     %s\n  reference %s" % (s, h, name, v, e[name], {n_: int(getattr(g, n_)) for n_ in COMPARED}, {n_: e[n_] for n_ in COMPARED}); break
                    if why:
                        break
                    cg = [int(g.cigar[t]) for t in range(g.n_cigar)]
                    if cg != w.cigars[s][h].tolist():
                        why = "mate %d record %d: the CIGAR is %s, the reference's %s" % (s, h, cg, w.cigars[s][h].tolist()); break
                if why:
                    break
            if why:
                bad.append("%s\n  %s" % (K.describe(optname, f), why))
            compared += 1; rd += len(f.qlens)
    ctx.close(); idx.close()
    if len(sys.argv) > 3:                                                      # (by hand: every mismatch, in full)
        open(sys.argv[3], "w").write("\n".join(bad))
    print(json.dumps({"generated": len(fr), "compared": compared, "n_mismatch": len(bad), "mismatches": bad[:4], "counts": total, "tiles": tiles, "tile_wrong": tile_wrong, "batches": len(groups),
                      "seconds_cases": round(t_gen, 2), "seconds_stage": round(t_gpu, 2), "seconds": round(time.time() - t0, 2)}))


if __name__ == "__main__":
    main()

"""One configuration of tests/test_gpu_hits_directed.py, in a process of its own (the environment switches are read once per process): the directed
chain sets of tests/hits_cases.py through the host code and the kernels of the stage between chaining and extension (al_dbg_regs) against the
reference's functions (oracle/_ref/libhitref.so), fragment by fragment, mate by mate, hit by hit.

usage: hits_directed_child.py <option set> <align|map_only> <all|serial> [<file for all mismatches>]     (the environment carries AL_DBG, AL_REGS_SPLIT, AL_TEST_SCRUB)
The fragments go in batches by read lengths, as the chain test's do: a batch's longest read sizes the logf table.  Prints one JSON line: generated,
compared, the first mismatches in full, and the counts that say which kernels did the work, summed over the batches."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import hits_cases as K  # noqa: E402

# columns of the 28-word device record (AlReg)
D = {"id": 0, "cnt": 1, "rid": 2, "score": 3, "qs": 4, "qe": 5, "rs": 6, "re": 7, "parent": 8, "subsc": 9, "as": 10, "mlen": 11, "blen": 12, "n_sub": 13, "score0": 14, "hash": 15, "mapq": 16, "flags": 17}
FLAG_BITS = {"rev": (2, 1), "sam_pri": (4, 1), "seg_split": (7, 1), "seg_id": (8, 0xff)}
KNOWN = sum(m << s for s, m in FLAG_BITS.values())


def device_hits(rec, with_mapq):
    """The compared fields of device records, in the order of K.COMPARED (+ mapq), as int64 columns; `other`: every flag bit the stage must leave 0."""
    cols = []
    for n in K.COMPARED + (("mapq",) if with_mapq else ()):
        if n in FLAG_BITS:
            s, m = FLAG_BITS[n]; cols.append((rec[:, D["flags"]] >> np.uint32(s)) & np.uint32(m))
        elif n == "other":
            cols.append(rec[:, D["flags"]] & np.uint32(~KNOWN & 0xffffffff))
        else:
            cols.append(rec[:, D[n]])
    return np.stack(cols, axis=1).astype(np.uint32).view(np.int32).astype(np.int64) if len(rec) else np.zeros((0, len(cols)), dtype=np.int64)


def hit_anchors(seg_a, as_, cnt):
    """The anchors seg_a[as .. as + cnt) of every hit, hit after hit."""
    tot = int(cnt.sum())
    if tot == 0:
        return np.zeros((0, 2), dtype=np.uint64)
    start = np.repeat(as_, cnt); first = np.repeat(np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt)
    idx = start + (np.arange(tot) - first)
    if idx.min() < 0 or idx.max() >= len(seg_a):
        return None
    return seg_a[idx]


def main():
    optname, mode, which = sys.argv[1], sys.argv[2], sys.argv[3]
    import airlift_amd as A
    o = K.OPTION_SETS[optname]
    t0 = time.time()
    fr = K.cases(optname)
    hashes, want = K.reference(optname)
    ids_all = [i for i, f in enumerate(fr) if which == "all" or len(f.u) <= K.SERIAL_MAX_CHAINS]
    t_gen = time.time() - t0
    groups = {}
    for i in ids_all:
        groups.setdefault(fr[i].qlens, []).append(i)
    rng = np.random.default_rng(3)
    refs = [bytes(b"ACGT"[c] for c in rng.integers(0, 4, 4000)) for _ in range(2)]
    idx = A.Index(seqs=refs, names=[b"chr", b"chr2"], k=o.k, w=11)
    m = idx.mo
    m.mask_level, m.pri_ratio, m.best_n, m.max_gap, m.max_gap_ref, m.max_frag_len, m.min_chain_score, m.a, m.b = o.mask_level, o.pri_ratio, o.best_n, o.max_gap, o.max_gap_ref, o.max_frag_len, o.min_chain_score, o.a, o.b
    if mode == "map_only":
        m.flag = (m.flag & ~(A.AL_F_CIGAR | 0x008)) | A.AL_F_OUT_PAF
    ctx = A.Context(idx)
    with_mapq = mode == "map_only"
    cmp_cols = [K.FIELDS.index(n) for n in K.COMPARED + (("mapq",) if with_mapq else ())]
    bad = []; compared = 0; total = {}; n0_kinds = {"f1": 0, "f2": 0, "f3": 0, "done": 0, "unset": 0, "kept": 0}; fast = 0; alias_f3 = 0; light = wave = 0
    t_gpu = 0.0; log_n_first = 0
    for qlens, ids in groups.items():
        n = len(ids); ns = len(qlens)
        ctx.upload([ns] * n, [b"A" * L for _ in ids for L in qlens], [K.frag_name(i) for i in ids for _ in qlens])
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
        r = ctx.regs(nu, u, uo, chained, a_off, rep)
        t_gpu += time.time() - t1
        for k_, v in r["counts"].items():
            total[k_] = max(total.get(k_, 0), v) if k_ in ("log_n", "select_ran") else total.get(k_, 0) + v
        log_n_first = c_first = r["counts"]["log_n"] if not total.get("batches_done") else log_n_first
        total["batches_done"] = total.get("batches_done", 0) + 1
        c = r["counts"]; lb = [c["lb5"], c["lb65"], c["lb257"], c["lb1025"], c["lb2049"], c["lb4097"], c["lb8193"], n if c["select_ran"] else 0]
        for t, name in enumerate(("class64", "class256", "class1024", "class2048", "class4096", "class8192", "class_above")):
            total[name] = total.get(name, 0) + (lb[t + 1] - lb[t] if c["select_ran"] else 0)
        recs = r["dense"] if with_mapq else r["regs"]
        got = device_hits(recs, with_mapq)
        if with_mapq and not np.array_equal(device_hits(r["regs"], False), got[:, :len(K.COMPARED)]):
            bad.append("reads %s: the dense map-only output differs from the per-mate hits in more than the MAPQ" % (qlens,))
        off = np.concatenate([[0], np.cumsum(r["reg_cnt"].astype(np.int64))])
        for j, i in enumerate(ids):
            f, w = fr[i], want[i]
            v = int(r["regs_n0"][j])
            n0_kinds["f1" if v == 0xfffffff1 else "f2" if v == 0xfffffff2 else "f3" if v == 0xfffffff3 else "done" if v == 0xfffffffe else "unset" if v == 0xffffffff else "kept"] += 1
            alias_f3 += v == 0xfffffff3 and sum(f.qlens) <= 65535
            fast += ns == 2 and len(f.u) == 1
            why = None
            if int(r["frag_hash"][j]) != hashes[i]:
                why = "the fragment's hash is %08x, the reference's %08x" % (int(r["frag_hash"][j]), hashes[i])
            for s in range(ns):
                if why:
                    break
                rd = j * ns + s; cnt = int(r["reg_cnt"][rd]); wb = (w.C if with_mapq else w.B)[s]
                light += 0 < cnt <= K.MO_LIGHT; wave += cnt > K.MO_LIGHT
                if cnt != len(wb):
                    why = "mate %d has %d hits, the reference %d" % (s, cnt, len(wb)); break
                g = got[off[rd]:off[rd] + cnt]; ww = wb[:, cmp_cols].astype(np.int64)
                if not np.array_equal(g, ww):
                    h, col = (int(x[0]) for x in np.nonzero(g != ww)); names = K.COMPARED + ("mapq",)
                    why = "mate %d hit %d: %s is %d, the reference's %d\n  stage     %s\n  reference %s" % (s, h, names[col], g[h, col], ww[h, col], dict(zip(names, g[h].tolist())), dict(zip(names, ww[h].tolist()))); break
                seg = r["seg_a"][int(a_off[j]) + (int(r["seg_na"][j * ns]) if s else 0):int(a_off[j + 1])]
                ga = hit_anchors(seg, recs[off[rd]:off[rd] + cnt, D["as"]].astype(np.int64), recs[off[rd]:off[rd] + cnt, D["cnt"]].astype(np.int64))
                if ga is None or not np.array_equal(ga, w.anch[s]):
                    why = "mate %d: the hits' anchors differ from the reference's" % s; break
            if why:
                bad.append("%s\n  regs_n0 %08x: %s" % (K.describe(optname, f, limit=6), v, why))
            compared += 1
    ctx.close(); idx.close()
    if len(sys.argv) > 4:                                                   # (by hand: every mismatch, in full)
        open(sys.argv[4], "w").write("\n".join(bad))
    print(json.dumps({"generated": len(ids_all), "listed": len(fr), "compared": compared, "n_mismatch": len(bad), "mismatches": bad[:4], "counts": total, "regs_n0": n0_kinds, "alias_f3": int(alias_f3), "one_chain_pairs": int(fast),
                      "log_n_first_batch": log_n_first, "first_batch": list(next(iter(groups))), "mates_light": int(light), "mates_wave": int(wave), "batches": len(groups), "chains_max": max(len(fr[i].u) for i in ids_all), "seconds_cases": round(t_gen, 2), "seconds_stage": round(t_gpu, 2),
                      "seconds": round(time.time() - t0, 2)}))


if __name__ == "__main__":
    main()

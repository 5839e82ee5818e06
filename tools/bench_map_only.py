#!/usr/bin/env python3
"""What a map-only step (AL_F_OUT_PAF without AL_F_CIGAR: no extension DP) costs next to the aligned step of the same build, on the
workload bench.py measures (C4: 1 M pairs of 150 bp against a human-sized reference), with the resident-batch API as bench.py's
resident leg uses it: one upload, then al_batch_run per step, per-stage times from the AlStage events.  bench.py is not touched;
its workload generator is imported.

    python tools/bench_map_only.py [--config c4] [--pairs 1000000] [--steps 5] [--warmup 2] [--text DIR]

Prints one JSON line: ms per step and per stage for both modes, the records each produced, device bytes each context held.
--text DIR: also writes the pairs as FASTQ into DIR and runs the command line under `rocprofv3 --kernel-trace --stats` three times
(-a, --paf -c, --paf), for the time of the text kernels (k_sam_len + k_sam_write + k_sam_bulk against k_paf_len + k_paf_write) and of
k_map_only itself; the per-kernel totals are added to the JSON line."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def run_mode(A, L, idx, arr, a, map_only):
    keep = idx.mo.flag
    if map_only:
        idx.mo.flag = (idx.mo.flag & ~(A.AL_F_CIGAR | 0x008)) | A.AL_F_OUT_PAF
    ctx = A.Context(idx, device=0)
    idx.mo.flag = keep
    L.al_ctx_set_threads(ctx.h, min(32, os.cpu_count() or 1))
    L.al_ctx_set_no_taps.argtypes = [C.c_void_p, C.c_int]; L.al_ctx_set_no_taps.restype = None
    L.al_ctx_set_no_taps(ctx.h, 1)
    import torch
    nf = a.pairs
    n_segs = (C.c_int * nf)(*([2] * nf)); qlens = (C.c_int * (2 * nf))(*([a.read_len] * (2 * nf)))
    free0 = torch.cuda.mem_get_info(0)[0]
    if L.al_batch_upload_flat(ctx.h, nf, n_segs, qlens, arr.ctypes.data_as(C.c_char_p), b"realigned_", 0) != 0:
        raise SystemExit("upload failed")
    ctx.n_frag, ctx.n_reads = nf, 2 * nf
    for _ in range(a.warmup):
        ctx.run()
    torch.cuda.synchronize()
    stage = np.zeros(40); t0 = time.perf_counter()
    for _ in range(a.steps):
        ctx.run()
        st = ctx.stat()
        stage += np.array(list(st.ms_kernel))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    held = free0 - torch.cuda.mem_get_info(0)[0]
    n_regs = (C.c_int * (2 * nf))(); regs = (C.POINTER(A.Reg) * (2 * nf))(); rep = (C.c_int * nf)()
    if L.al_batch_fetch(ctx.h, n_regs, regs, rep) != 0:
        raise SystemExit("fetch failed")
    names = [L.al_stage_name(i).decode() for i in range(st.n_stage)]
    out = {"ms_per_step": 1e3 * dt / a.steps, "reads_per_s": 2.0 * nf * a.steps / dt, "stages_ms": {names[i]: float(stage[i] / a.steps) for i in range(st.n_stage)},
           "records": int(sum(n_regs)), "cigar_words": int(st.n_cigar), "device_bytes_held_by_the_batch": int(held)}
    ctx.close()
    return out


def text_kernels(d, arr, a, ref_fa):
    from bench import write_fastq_sample
    os.makedirs(d, exist_ok=True)
    fq = [os.path.join(d, "reads_%d.fq" % (m + 1)) for m in range(2)]
    for m in range(2):
        write_fastq_sample(fq[m], arr, m)
    cli = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
    res = {}
    for tag, opts in (("sam", ["-a"]), ("paf_c", ["--paf", "-c"]), ("paf_map_only", ["--paf"])):
        od = os.path.join(d, "prof_" + tag)
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", od, "--output-format", "csv", "--", cli, "-x", "sr", "-t", "16"] + opts + ["-o", os.path.join(d, "out." + tag), ref_fa] + fq,
                           capture_output=True, timeout=900, env=dict(os.environ, AL_NO_FAST_EXIT="1", AL_TIMING="1"))
        if r.returncode != 0:
            raise SystemExit("command line under rocprofv3 failed (%s): %s" % (tag, r.stderr.decode()[-1500:]))
        per = {}
        for fn in glob.glob(os.path.join(od, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(fn)):
                nm = row.get("Name", "")
                for k in ("k_sam_len", "k_sam_write", "k_sam_bulk", "k_paf_len", "k_paf_write", "k_map_only_wave", "k_map_only", "k_compact", "k_regs(", "k_ext_prep(", "k_ext_finish("):
                    if k in nm and not (k == "k_map_only" and "wave" in nm):
                        e = per.setdefault(k.rstrip("("), {"calls": 0, "total_ms": 0.0}); e["calls"] += int(row.get("Calls", 0)); e["total_ms"] += float(row.get("TotalDurationNs", 0)) / 1e6
        res[tag] = {"kernels": per, "output_bytes": os.path.getsize(os.path.join(d, "out." + tag)),
                    "pipeline": [l for l in r.stderr.decode().split("\n") if "stream pipeline:" in l][:1]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4"); ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--text", metavar="DIR", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    import gen_synth as g
    import airlift_amd as A
    from bench import make_workload
    L = A.load()
    L.al_batch_upload_flat.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_char_p, C.c_int64]; L.al_batch_upload_flat.restype = C.c_int
    a.read_len = g.CONFIGS[a.config][1]["read_len"]
    tmp = a.text or tempfile.mkdtemp(prefix="al_mo_")
    os.makedirs(tmp, exist_ok=True)
    ref = g.build_reference(a.config)
    ref_fa = os.path.join(tmp, "ref.fa"); g.write_fasta(ref_fa, ref)
    idx = A.Index(fasta=ref_fa, on_device=0)
    arr = make_workload(a.config, 0, a.pairs, a.read_len, 20261002, ref)
    out = {"config": a.config, "pairs": a.pairs, "steps": a.steps, "warmup": a.warmup}
    out["aligned"] = run_mode(A, L, idx, arr, a, False)
    out["map_only"] = run_mode(A, L, idx, arr, a, True)
    ext = [k for k in out["aligned"]["stages_ms"] if k.startswith("ext_")] + ["compact"]
    out["aligned_extension_ms"] = sum(out["aligned"]["stages_ms"][k] for k in ext)
    out["map_only_stage_ms"] = out["map_only"]["stages_ms"].get("map_only")
    idx.close()
    if a.text:
        out["text"] = text_kernels(a.text, arr, a, ref_fa)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

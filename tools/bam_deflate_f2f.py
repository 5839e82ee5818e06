#!/usr/bin/env python3
"""BAM output file to file, host deflate against --gpu-deflate (profiles/r11_gpu_deflate.json).

The first PAIRS pairs of the C4 workload (tools/gen_synth.py) as two FASTQ files in memory-backed storage -> airlift-align -ax sr -t 16 ... -o FILE,
AL_TIMING=1.  The parent commit's build (--parent DIR: the directory that holds its bin/ and lib/) and this tree alternate: one warm-up round that
is recorded as rep 0 and not reported, then --reps rounds.  Per run: wall seconds, the driver's pipeline seconds, the deflate seconds (with
--gpu-deflate: kernels by HIP events and transfers apart), file size and md5.  Every process runs under a time limit; the series stops at the
first run that fails.

    python tools/bam_deflate_f2f.py --parent /path/to/parent/airlift_amd --out profiles/r11_gpu_deflate.json
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


FIELDS = ("pipeline_s = the AL_TIMING total of the driver's summary line; deflate_s = AlBgzf::t_deflate (host: wall time of the zlib worker rounds; --gpu-deflate: "
          "uploads, kernels, downloads and writes of the members); deflate_kernel_s = k_deflate + k_dfl_offsets + k_dfl_pack by HIP events, deflate_transfer_s = the copies' "
          "wall time; resident_blocks = blocks compressed where the batch lay in device memory; after_last_batch_s = sort / merge / last blocks after the last batch; "
          "rep 0 is the warm-up round and is not reported")


def md5(path):
    h = hashlib.md5()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def first(rx, text, cast=float):
    m = re.search(rx, text)
    return cast(m.group(1)) if m else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="airlift_amd directory of the parent commit's build (bin/airlift-align, lib/libairlift.so)")
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--dir", default="/dev/shm/al_r11")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_gpu_deflate.json"))
    ap.add_argument("--limit", type=int, default=120, help="seconds a run may take")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    ref_fa, f1, f2 = (os.path.join(a.dir, n) for n in ("ref.fa", "r_1.fq", "r_2.fq"))
    if not all(os.path.exists(p) for p in (ref_fa, f1, f2)):
        import gen_synth as g
        sys.path.insert(0, ROOT)
        import bench                                               # the workload is bench.py's: same fragments, same names
        t0 = time.time()
        ref = g.build_reference("c4"); print("reference built in %.0f s" % (time.time() - t0), flush=True)
        g.write_fasta(ref_fa, ref); print("reference written at %.0f s" % (time.time() - t0), flush=True)
        arr = bench.make_workload("c4", 0, a.pairs, 150, 20261002, ref)
        bench.write_fastq_fast(f1, arr, 0); bench.write_fastq_fast(f2, arr, 1)
        del ref, arr
        print("workload written in %.0f s" % (time.time() - t0), flush=True)
    trees = {"parent": os.path.join(a.parent, "bin", "airlift-align"), "this": os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")}
    series = [("bam_l1", "parent", ["--bam", "-l", "1"]), ("bam_gpu", "this", ["--bam", "--gpu-deflate"]),
              ("bam_l5", "parent", ["--bam", "-l", "5"]), ("bam_l5", "this", ["--bam", "-l", "5"]),
              ("sorted_l5", "parent", ["--sorted-bam", "-l", "5"]), ("sorted_gpu", "this", ["--sorted-bam", "--gpu-deflate"]),
              ("bam_l1", "this", ["--bam", "-l", "1"])]
    runs = []
    out = os.path.join(a.dir, "out.bam")
    for rep in range(a.reps + 1):
        for name, tree, opts in series:
            cmd = ["timeout", "-k", "10", str(a.limit), trees[tree], "-ax", "sr", "-t", str(a.threads)] + opts + ["-o", out, ref_fa, f1, f2]
            t0 = time.time()
            r = subprocess.run(cmd, stderr=subprocess.PIPE, env=dict(os.environ, AL_PG_PLAIN="1", AL_TIMING="1"))
            wall = time.time() - t0
            err = r.stderr.decode(errors="replace")
            if r.returncode != 0:
                print("run failed (%d): %s\n%s" % (r.returncode, " ".join(cmd), err[-3000:]), flush=True)
                json.dump({"failed": cmd, "rc": r.returncode, "runs": runs}, open(a.out, "w"), indent=1)
                return 1
            rec = dict(rep=rep, output=name, tree=tree, wall_s=round(wall, 3),
                       pipeline_s=first(r"stream pipeline: .*; total ([0-9.]+) s", err) or first(r"pipeline lane 0 .*; total ([0-9.]+) s", err),
                       index_build_s=first(r"index build ([0-9.]+) s", err),
                       deflate_s=first(r"BAM output: deflate \([^)]*\) ([0-9.]+) s in all", err),
                       deflate_kernel_s=first(r"deflate \(device[^\n]*kernels ([0-9.]+) s", err), deflate_transfer_s=first(r"deflate \(device[^\n]*transfers ([0-9.]+) s", err),
                       blocks=first(r"deflate \(device[^\n]*; ([0-9]+) blocks,", err, int), stored_blocks=first(r"deflate \(device[^\n]* ([0-9]+) stored", err, int),
                       resident_blocks=first(r"deflate \(device[^\n]*blocks, ([0-9]+) of them", err, int),
                       after_last_batch_s=first(r"after the last batch ([0-9.]+) s", err),
                       mappers_run_s=first(r"mappers \(sum\): setup [0-9.]+ run ([0-9.]+)", err), writer_s=first(r"; writer ([0-9.]+);", err),
                       bytes=os.path.getsize(out), md5=md5(out))
            if rec["deflate_kernel_s"]:
                rec["kernel_GBps_of_input"] = round(rec["blocks"] * 0xff00 / rec["deflate_kernel_s"] / 1e9, 2)
            runs.append(rec)
            print(json.dumps(rec), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump({"what": __doc__.strip().split("\n\n")[1], "fields": FIELDS, "pairs": a.pairs, "threads": a.threads, "runs": runs}, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""BAM file to lifted BAM and BED: `lift` on the device, with --gpu-deflate, and its host twin on --threads threads (profiles/r23_lift.json).

The input is the BAM of the r13 series (tools/bam_inflate_f2f.py): the first PAIRS pairs of the C4 workload (tools/gen_synth.py) mapped with -ax sr --sorted-bam
-l 5, in memory-backed storage (made here when it is not there yet), and the chain file tools/chain_beds_f2f.py makes for C4: one '+' chain per contig with
--windows gaps of 5 kb at even distances.  `lift` then runs in three forms: on the device, on the device with --gpu-deflate, and --host -t THREADS.  One warm-up
round that is recorded as rep 0 and not reported, then --reps rounds, the forms alternating.  Per run: wall seconds, the pieces of the AL_TIMING line, the three
counts; once per form the md5 of the inflated output BAM and of the BED.  Every process runs under a time limit; the series stops at the first run that fails.
There is no parent form of this command, and no time is a pass criterion.

    python tools/lift_f2f.py --out profiles/r23_lift.json
"""
import argparse
import gzip
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")

FIELDS = ("wall_s = the process, start to exit; the rest is the AL_TIMING line of lift: read_s = pread of the pieces; up_s = the copies up and the waits around the inflate launches; "
          "inflate_s = k_inflate by HIP events (host twin: wall time of its inflate rounds); walk_s = k_bam_walk; lift_s = k_lift, the two scans and k_lift_gather; down_s = the copies down; "
          "deflate_s = AlBgzf's compression, device or host threads; walk_GBps = inflated bytes / walk_s; rep 0 is the warm-up round and is not reported")


def first(rx, text, cast=float):
    m = re.search(rx, text)
    return cast(m.group(1)) if m else None


def md5_inflated(path):
    h = hashlib.md5()
    with gzip.open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--windows", type=int, default=2000)
    ap.add_argument("--dir", default="/dev/shm/al_r13")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_lift.json"))
    ap.add_argument("--limit", type=int, default=180, help="seconds a run may take")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    ref_fa, f1, f2, bam, chain = (os.path.join(a.dir, n) for n in ("ref.fa", "r_1.fq", "r_2.fq", "reads.bam", "c4.chain"))
    if not os.path.exists(bam) or not os.path.exists(chain):
        import gen_synth as g
        sys.path.insert(0, ROOT)
        import bench                                                   # the workload is bench.py's: same fragments, same names
        from chain_beds_f2f import windows_chain
        t0 = time.time()
        ref = g.build_reference("c4"); g.write_fasta(ref_fa, ref); print("reference written at %.0f s" % (time.time() - t0), flush=True)
        text, kept, skipped = windows_chain(ref, a.windows, 5000, 160)
        open(chain, "w").write(text)
        if not os.path.exists(bam):
            arr = bench.make_workload("c4", 0, a.pairs, 150, 20261002, ref)
            bench.write_fastq_fast(f1, arr, 0); bench.write_fastq_fast(f2, arr, 1)
            del arr
            print("workload written in %.0f s" % (time.time() - t0), flush=True)
            cmd = ["timeout", "-k", "10", str(a.limit), CLI, "-ax", "sr", "-t", str(a.threads), "--sorted-bam", "-l", "5", "-o", bam, ref_fa, f1, f2]
            r = subprocess.run(cmd, stderr=subprocess.PIPE, env=dict(os.environ, AL_PG_PLAIN="1"))
            if r.returncode != 0:
                print("the mapping run failed (%d)\n%s" % (r.returncode, r.stderr.decode(errors="replace")[-3000:]), flush=True)
                return 1
            os.remove(f1); os.remove(f2)
            print("BAM written at %.0f s" % (time.time() - t0), flush=True)
        del ref
    series = [("device", []), ("device_gpu_deflate", ["--gpu-deflate"]), ("host_twin", ["--host"])]
    runs, sums = [], {}
    for rep in range(a.reps + 1):
        for name, opts in series:
            out, bed = os.path.join(a.dir, "lift_%s.bam" % name), os.path.join(a.dir, "lift_%s.bed" % name)
            cmd = ["timeout", "-k", "10", str(a.limit), CLI, "lift", "--chain", chain, "-o", out, "--unmapped-bed", bed, "-l", "5", "-t", str(a.threads)] + opts + [bam]
            t0 = time.time()
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, AL_TIMING="1"))
            wall = time.time() - t0
            err = r.stderr.decode(errors="replace")
            if r.returncode != 0:
                print("run failed (%d): %s\n%s" % (r.returncode, " ".join(cmd), err[-3000:]), flush=True)
                json.dump({"failed": cmd, "rc": r.returncode, "runs": runs}, open(a.out, "w"), indent=1)
                return 1
            rec = dict(rep=rep, form=name, wall_s=round(wall, 3), backend=first(r"lift: '[^']*' \(([^)]*)\)", err, str), pieces=first(r"([0-9]+) pieces", err, int), bytes_in=first(r"([0-9]+) bytes in", err, int),
                       kept=first(r"([0-9]+) kept", err, int), unlifted=first(r"([0-9]+) unlifted", err, int), unmapped_kept=first(r"([0-9]+) unmapped kept", err, int),
                       read_s=first(r"file read ([0-9.]+) s", err), up_s=first(r"copy up ([0-9.]+) s", err), inflate_s=first(r"inflate ([0-9.]+) s", err), walk_s=first(r"walk ([0-9.]+) s", err),
                       lift_s=first(r"lift and gather ([0-9.]+) s", err), down_s=first(r"copy down ([0-9.]+) s", err), deflate_s=first(r"deflate ([0-9.]+) s, wall", err), held=first(r"held at return: ([0-9]+)", err, int),
                       out_bytes=os.path.getsize(out), bed_bytes=os.path.getsize(bed))
            if rec["walk_s"]:
                rec["walk_GBps"] = round(rec["bytes_in"] / rec["walk_s"] / 1e9, 2)
            if rec["inflate_s"]:
                rec["inflate_GBps"] = round(rec["bytes_in"] / rec["inflate_s"] / 1e9, 2)
            if rep == a.reps:
                sums[name] = dict(bam_md5=md5_inflated(out), bed_md5=hashlib.md5(open(bed, "rb").read()).hexdigest())
            os.remove(out); os.remove(bed)
            runs.append(rec)
            print(json.dumps(rec), flush=True)
            summ = {n: dict(wall_s_median=round(statistics.median(x["wall_s"] for x in runs if x["form"] == n and x["rep"]), 3), wall_s_all=[x["wall_s"] for x in runs if x["form"] == n and x["rep"]])
                    for n, _ in series if any(x["form"] == n and x["rep"] for x in runs)}
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump({"what": __doc__.strip().split("\n\n")[1], "fields": FIELDS, "pairs": a.pairs, "threads": a.threads, "bam_bytes": os.path.getsize(bam), "chain_windows": a.windows,
                       "summary": summ, "output_md5": sums, "runs": runs}, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""BAM file to BAI: `bam-index` on the device against its host twin on --threads threads, and `merge` with and without --write-index (DESIGN.md section 5,
profiles/r26_index.json).

The input is the `lift --sorted` output of the r24 workload: the 2 M-pair BAM of the C4 workload (tools/lift_f2f.py makes it when it is not there yet) lifted across
the C4 chain file with --sorted, in memory-backed storage.  Forms, alternating: (a) `bam-index` on the device, (b) `bam-index --host -t THREADS`, (c) `merge` of the
lifted BAM with itself (two inputs, so the output is twice the size), (d) the same with --write-index.  One warm-up round that is
recorded as rep 0 and not reported, then --reps rounds.  Per run: process wall seconds and the shares of the AL_TIMING line; once per form the md5 of the index.
Every process runs under a time limit; the series stops at the first run that fails.  There is no parent form of this command and no samtools to compare with: the
two forms are reported side by side, and no time is a pass criterion.

    python tools/index_f2f.py --out profiles/r26_index.json
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
from lift_f2f import first  # noqa: E402

FIELDS = ("wall_s = the process, start to exit; the rest is the AL_TIMING line of bam-index: read_s = pread of the pieces; up_s = the copies up and the waits around the inflate launches; "
          "inflate_s = k_inflate by HIP events (host twin: wall time of its inflate rounds); walk_s = k_bam_walk; key_s = k_bai_key, k_bai_heads, the scan, k_bai_rows, k_bai_lin and the rows' "
          "copy down (host twin: its loop over the records); assemble_s = the tables' copy down, the host's sort and join of the rows, the file's write; walk_GBps / inflate_GBps = inflated "
          "bytes over those seconds; the merge forms: wall_s alone, and index_wall_s = the wall of the bam-index line the same process prints; rep 0 is the warm-up round and is not reported")


def index_fields(err):
    """the fields of the process's `[airlift] bam-index:` line"""
    line = ([l for l in err.split("\n") if l.startswith("[airlift] bam-index:")] or [""])[-1]
    rec = dict(backend=first(r"\(([^)]*)\):", line, str), records=first(r"([0-9]+) records", line, int), pieces=first(r"([0-9]+) pieces", line, int), bytes_in=first(r"([0-9]+) bytes in", line, int),
               chunks=first(r"([0-9]+) chunks", line, int), bai_bytes=first(r"([0-9]+) bytes of index", line, int), read_s=first(r"file read ([0-9.]+) s", line), up_s=first(r"copy up ([0-9.]+) s", line),
               inflate_s=first(r"inflate ([0-9.]+) s", line), walk_s=first(r"walk ([0-9.]+) s", line), key_s=first(r"keys ([0-9.]+) s", line), assemble_s=first(r"assemble ([0-9.]+) s", line),
               index_wall_s=first(r"wall ([0-9.]+) s", line), held=first(r"held at return: ([0-9]+)", line, int))
    if rec["walk_s"]:
        rec["walk_GBps"] = round(rec["bytes_in"] / rec["walk_s"] / 1e9, 2)
    if rec["inflate_s"]:
        rec["inflate_GBps"] = round(rec["bytes_in"] / rec["inflate_s"] / 1e9, 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--dir", default="/dev/shm/al_r13")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_index.json"))
    ap.add_argument("--limit", type=int, default=180, help="seconds a run may take")
    a = ap.parse_args()
    bam, chain, lifted = (os.path.join(a.dir, n) for n in ("reads.bam", "c4.chain", "lifted_sorted.bam"))
    if not os.path.exists(bam) or not os.path.exists(chain):
        print("the r23 input is not in %s: make it with tools/lift_f2f.py --reps 0" % a.dir, flush=True)
        return 1
    if not os.path.exists(lifted):
        cmd = ["timeout", "-k", "10", str(a.limit), CLI, "lift", "--chain", chain, "--sorted", "-o", lifted, "--unmapped-bed", os.path.join(a.dir, "lifted_sorted.bed"), "-l", "5", "-t", str(a.threads), bam]
        r = subprocess.run(cmd, stderr=subprocess.PIPE)
        if r.returncode != 0:
            print("lift --sorted failed (%d)\n%s" % (r.returncode, r.stderr.decode(errors="replace")[-3000:]), flush=True)
            return 1
    merged = os.path.join(a.dir, "index_merged.bam")
    series = [("a_index_device", ["bam-index", "-t", str(a.threads), lifted], lifted + ".bai"), ("b_index_host", ["bam-index", "--host", "-t", str(a.threads), lifted], lifted + ".bai"),
              ("c_merge", ["merge", "-o", merged, "-l", "5", "-t", str(a.threads), lifted, lifted], None),
              ("d_merge_write_index", ["merge", "--write-index", "-o", merged, "-l", "5", "-t", str(a.threads), lifted, lifted], merged + ".bai")]
    runs, sums = [], {}
    for rep in range(a.reps + 1):
        for name, args, bai in series:
            cmd = ["timeout", "-k", "10", str(a.limit), CLI] + args
            t0 = time.time()
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, AL_TIMING="1"))
            wall = time.time() - t0
            err = r.stderr.decode(errors="replace")
            if r.returncode != 0:
                print("run failed (%d): %s\n%s" % (r.returncode, " ".join(cmd), err[-3000:]), flush=True)
                json.dump({"failed": cmd, "rc": r.returncode, "runs": runs}, open(a.out, "w"), indent=1)
                return 1
            rec = dict(rep=rep, form=name, wall_s=round(wall, 3))
            if bai:
                rec.update(index_fields(err))
                if rep == a.reps:
                    sums[name] = dict(bai_md5=hashlib.md5(open(bai, "rb").read()).hexdigest(), bai_bytes=os.path.getsize(bai))
                os.remove(bai)
            if os.path.exists(merged):
                os.remove(merged)
            runs.append(rec)
            print(json.dumps(rec), flush=True)
            summ = {n: dict(wall_s_median=round(statistics.median(x["wall_s"] for x in runs if x["form"] == n and x["rep"]), 3), wall_s_all=[x["wall_s"] for x in runs if x["form"] == n and x["rep"]])
                    for n, _, _ in series if any(x["form"] == n and x["rep"] for x in runs)}
            noise = max([max(v["wall_s_all"]) - min(v["wall_s_all"]) for v in summ.values()] or [0])
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump({"what": __doc__.strip().split("\n\n")[1], "fields": FIELDS, "threads": a.threads, "bam_bytes": os.path.getsize(lifted), "largest_spread_within_a_form_s": round(noise, 3),
                       "summary": summ, "outputs": sums, "runs": runs}, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

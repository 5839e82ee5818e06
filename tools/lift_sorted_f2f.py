#!/usr/bin/env python3
"""BAM file to lifted BAM in coordinate order: `lift --sorted` against `lift`, and this tree's `lift` against the parent commit's (DESIGN.md section 5,
profiles/r24_lift_sorted.json).

The input is the one of the r23 series (tools/lift_f2f.py, which makes it when it is not there yet): the 2 M-pair BAM of the C4 workload, coordinate-sorted, and
the C4 chain file with 2 000 gaps, in memory-backed storage.  Five forms, alternating: (a) the parent commit's `lift` (--parent-cli: a build of the commit before
this feature), (b) this tree's `lift`, (c) `lift --sorted`, (d) `lift --sorted --gpu-deflate`, (e) `lift --sorted --host -t THREADS`.  One warm-up round that is
recorded as rep 0 and not reported, then --reps rounds.  Per run: process wall seconds, the pieces of the AL_TIMING lines (for --sorted: pieces in order and
sorted, runs chained, spills, seconds of the device sort, the permuted gather and the host merge); once per form the md5 of the inflated output and of the BED,
and for the sorted forms whether the keys of the output are in order.  Every process runs under a time limit; the series stops at the first run that fails.  The
verdicts follow the noise rule: a difference counts only if the smallest gap between two forms exceeds the largest difference between two runs of one form.

    python tools/lift_sorted_f2f.py --parent-cli /path/to/parent/airlift-align --out profiles/r24_lift_sorted.json
"""
import argparse
import gzip
import hashlib
import json
import os
import statistics
import struct
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
from lift_f2f import first  # noqa: E402


def inspect(path):
    """md5 of the inflated BAM, its record count, whether refID << 32 | pos (~0 without a refID) never descends, and the md5 of the sorted record multiset's
    per-record md5s (equal for two files that hold the same records in any order)"""
    h = hashlib.md5(); blob = gzip.open(path, "rb").read(); h.update(blob)
    l_text = struct.unpack_from("<i", blob, 4)[0]; p = 8 + l_text
    n_ref = struct.unpack_from("<i", blob, p)[0]; p += 4
    for _ in range(n_ref):
        p += 8 + struct.unpack_from("<i", blob, p)[0]
    last, ordered, n, acc = -1, True, 0, 0
    while p < len(blob):
        bs, rid, pos = struct.unpack_from("<iii", blob, p)
        k = (1 << 64) - 1 if rid < 0 else rid << 32 | (pos & 0xffffffff)
        ordered = ordered and k >= last; last = k; n += 1
        acc = (acc + int.from_bytes(hashlib.md5(blob[p:p + 4 + bs]).digest(), "little")) & ((1 << 128) - 1)
        p += 4 + bs
    return dict(bam_md5=h.hexdigest(), records=n, in_key_order=ordered, record_multiset="%032x" % acc, header_so=first(r"SO:([a-z]+)", blob[8:8 + l_text].decode(errors="replace"), str))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-cli", required=True, help="airlift-align of the commit before lift --sorted")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--dir", default="/dev/shm/al_r13")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_lift_sorted.json"))
    ap.add_argument("--limit", type=int, default=180, help="seconds a run may take")
    a = ap.parse_args()
    bam, chain = os.path.join(a.dir, "reads.bam"), os.path.join(a.dir, "c4.chain")
    if not os.path.exists(bam) or not os.path.exists(chain):
        print("the r23 input is not in %s: make it with tools/lift_f2f.py --reps 0" % a.dir, flush=True)
        return 1
    series = [("a_parent_lift", a.parent_cli, []), ("b_lift", CLI, []), ("c_sorted", CLI, ["--sorted"]), ("d_sorted_gpu_deflate", CLI, ["--sorted", "--gpu-deflate"]),
              ("e_sorted_host", CLI, ["--sorted", "--host"])]
    runs, sums = [], {}
    for rep in range(a.reps + 1):
        for name, cli, opts in series:
            out, bed = os.path.join(a.dir, "lifts_%s.bam" % name), os.path.join(a.dir, "lifts_%s.bed" % name)
            cmd = ["timeout", "-k", "10", str(a.limit), cli, "lift", "--chain", chain, "-o", out, "--unmapped-bed", bed, "-l", "5", "-t", str(a.threads)] + opts + [bam]
            t0 = time.time()
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, AL_TIMING="1"))
            wall = time.time() - t0
            err = r.stderr.decode(errors="replace")
            if r.returncode != 0:
                print("run failed (%d): %s\n%s" % (r.returncode, " ".join(cmd), err[-3000:]), flush=True)
                json.dump({"failed": cmd, "rc": r.returncode, "runs": runs}, open(a.out, "w"), indent=1)
                return 1
            rec = dict(rep=rep, form=name, wall_s=round(wall, 3), backend=first(r"lift: '[^']*' \(([^)]*)\)", err, str), pieces=first(r"([0-9]+) pieces,", err, int), kept=first(r"([0-9]+) kept", err, int),
                       unlifted=first(r"([0-9]+) unlifted", err, int), inflate_s=first(r"inflate ([0-9.]+) s", err), walk_s=first(r"walk ([0-9.]+) s", err), lift_s=first(r"lift and gather ([0-9.]+) s", err),
                       down_s=first(r"copy down ([0-9.]+) s", err), deflate_s=first(r"deflate ([0-9.]+) s, wall", err), held=first(r"held at return: ([0-9]+)", err, int), out_bytes=os.path.getsize(out))
            if "--sorted" in opts:
                rec.update(pieces_in_order=first(r"([0-9]+) pieces in order", err, int), pieces_sorted=first(r"([0-9]+) pieces sorted", err, int), runs_chained=first(r"([0-9]+) chained", err, int),
                           spills=first(r"([0-9]+) spills", err, int), sort_s=first(r"; sort ([0-9.]+) s", err), permuted_gather_s=first(r"permuted gather ([0-9.]+) s", err), host_merge_s=first(r"host merge ([0-9.]+) s", err))
            if rep == a.reps:
                sums[name] = dict(inspect(out), bed_md5=hashlib.md5(open(bed, "rb").read()).hexdigest())
            os.remove(out); os.remove(bed)
            runs.append(rec)
            print(json.dumps(rec), flush=True)
            summ = {n: dict(wall_s_median=round(statistics.median(x["wall_s"] for x in runs if x["form"] == n and x["rep"]), 3), wall_s_all=[x["wall_s"] for x in runs if x["form"] == n and x["rep"]])
                    for n, _, _ in series if any(x["form"] == n and x["rep"] for x in runs)}
            noise = max([max(v["wall_s_all"]) - min(v["wall_s_all"]) for v in summ.values()] or [0])
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump({"what": __doc__.strip().split("\n\n")[1], "threads": a.threads, "bam_bytes": os.path.getsize(bam), "largest_spread_within_a_form_s": round(noise, 3),
                       "summary": summ, "outputs": sums, "runs": runs}, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

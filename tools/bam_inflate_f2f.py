#!/usr/bin/env python3
"""BAM input file to rows: the gzread reader against --gpu-inflate and its host-thread backend (profiles/r13_gpu_inflate.json).

The input is the BAM that tools/bam_deflate_f2f.py's sorted_l5 run writes: the first PAIRS pairs of the C4 workload (tools/gen_synth.py) mapped with
-ax sr --sorted-bam -l 5, in memory-backed storage (made here when it is not there yet), and a BED of --regions regions of 20 kb spread evenly over the
reference.  `extract-reads` then runs in three forms: the parent commit's build (--parent DIR: the directory that holds its bin/ and lib/), this tree
with --gpu-inflate, and this tree with --gpu-inflate on the reader's host backend (AL_TEST_INFLATE_HOST=1: zlib per member on --threads threads); a fourth
form repeats --gpu-inflate with pieces of 4 MB instead of the default 16 (AL_INFLATE_PIECE_KB), to show what the members in flight are worth.  One
warm-up round that is recorded as rep 0 and not reported, then --reps rounds, the forms alternating.  Per run: wall seconds, the AL_TIMING breakdown of
the reader, rows and their md5.  Every process runs under a time limit; the series stops at the first run that fails.

    python tools/bam_inflate_f2f.py --parent /path/to/parent/airlift_amd --out profiles/r13_gpu_inflate.json
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

FIELDS = ("wall_s = the process, start to exit; the rest is the reader's AL_TIMING line: file_read_s = pread of the pieces; h2d_s, kernel_s, d2h_s = HIP events around the "
          "copies up, k_inflate (CRC32 of every member included) and the copies down, summed over the pieces; host_inflate_s, crc_s = wall time of the zlib and crc32 worker "
          "rounds of the host backend; scan_s = the record loop without its waits for pieces, wait_s = those waits; kernel_GBps_out = bytes out / kernel_s; "
          "rep 0 is the warm-up round and is not reported")


def first(rx, text, cast=float):
    m = re.search(rx, text)
    return cast(m.group(1)) if m else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="airlift_amd directory of the parent commit's build (bin/airlift-align, lib/libairlift.so)")
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--regions", type=int, default=300)
    ap.add_argument("--dir", default="/dev/shm/al_r13")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_gpu_inflate.json"))
    ap.add_argument("--limit", type=int, default=120, help="seconds a run may take")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    this = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
    ref_fa, f1, f2, bam, bed = (os.path.join(a.dir, n) for n in ("ref.fa", "r_1.fq", "r_2.fq", "reads.bam", "regions.bed"))
    if not os.path.exists(bam):
        if not all(os.path.exists(p) for p in (ref_fa, f1, f2)):
            import gen_synth as g
            sys.path.insert(0, ROOT)
            import bench                                               # the workload is bench.py's: same fragments, same names
            t0 = time.time()
            ref = g.build_reference("c4"); g.write_fasta(ref_fa, ref); print("reference written at %.0f s" % (time.time() - t0), flush=True)
            arr = bench.make_workload("c4", 0, a.pairs, 150, 20261002, ref)
            bench.write_fastq_fast(f1, arr, 0); bench.write_fastq_fast(f2, arr, 1)
            del ref, arr
            print("workload written in %.0f s" % (time.time() - t0), flush=True)
        cmd = ["timeout", "-k", "10", str(a.limit), this, "-ax", "sr", "-t", str(a.threads), "--sorted-bam", "-l", "5", "-o", bam, ref_fa, f1, f2]
        r = subprocess.run(cmd, stderr=subprocess.PIPE, env=dict(os.environ, AL_PG_PLAIN="1"))
        if r.returncode != 0:
            print("the mapping run failed (%d)\n%s" % (r.returncode, r.stderr.decode(errors="replace")[-3000:]), flush=True)
            return 1
        os.remove(f1); os.remove(f2)
    if not os.path.exists(bed):
        seqs, name, n = [], None, 0
        for line in open(ref_fa):
            if line.startswith(">"):
                if name:
                    seqs.append((name, n))
                name, n = line[1:].split()[0], 0
            else:
                n += len(line) - 1
        seqs.append((name, n))
        total = sum(n for _, n in seqs); step = total // a.regions
        with open(bed, "w") as f:
            for k in range(a.regions):
                at = k * step
                for nm, n in seqs:
                    if at < n:
                        if at + 20000 < n:
                            f.write("%s\t%d\t%d\n" % (nm, at + 1, at + 20000))
                        break
                    at -= n
    trees = {"parent": os.path.join(a.parent, "bin", "airlift-align"), "this": this}
    series = [("gzread", "parent", [], {}), ("gpu_inflate", "this", ["--gpu-inflate", "-t", str(a.threads)], {}),
              ("host_threads", "this", ["--gpu-inflate", "-t", str(a.threads)], {"AL_TEST_INFLATE_HOST": "1"}),
              ("gpu_inflate_piece_4m", "this", ["--gpu-inflate", "-t", str(a.threads)], {"AL_INFLATE_PIECE_KB": "4096"})]
    runs = []
    for rep in range(a.reps + 1):
        for name, tree, opts, env in series:
            cmd = ["timeout", "-k", "10", str(a.limit), trees[tree], "extract-reads", "--noprune"] + opts + [bam, bed]
            t0 = time.time()
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, AL_TIMING="1", **env))
            wall = time.time() - t0
            err = r.stderr.decode(errors="replace")
            if r.returncode != 0:
                print("run failed (%d): %s\n%s" % (r.returncode, " ".join(cmd), err[-3000:]), flush=True)
                json.dump({"failed": cmd, "rc": r.returncode, "runs": runs}, open(a.out, "w"), indent=1)
                return 1
            rec = dict(rep=rep, form=name, tree=tree, wall_s=round(wall, 3), rows=r.stdout.count(b"\n"), md5=hashlib.md5(r.stdout).hexdigest(),
                       file_read_s=first(r"file read ([0-9.]+) s", err), h2d_s=first(r"H2D ([0-9.]+) s", err), kernel_s=first(r"kernels ([0-9.]+) s", err), d2h_s=first(r"D2H ([0-9.]+) s", err),
                       crc_s=first(r"CRC ([0-9.]+) s", err), host_inflate_s=first(r"host inflate ([0-9.]+) s", err), scan_s=first(r"record scan ([0-9.]+) s", err),
                       wait_s=first(r"\(\+ ([0-9.]+) s waiting", err), members=first(r"([0-9]+) members in", err, int), pieces=first(r"members in ([0-9]+) pieces", err, int),
                       bytes_in=first(r"([0-9]+) bytes in", err, int), bytes_out=first(r"([0-9]+) bytes out", err, int), host_pieces=first(r"([0-9]+) pieces on the host backend", err, int))
            if rec["kernel_s"]:
                rec["kernel_GBps_out"] = round(rec["bytes_out"] / rec["kernel_s"] / 1e9, 2)
            runs.append(rec)
            print(json.dumps(rec), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump({"what": __doc__.strip().split("\n\n")[1], "fields": FIELDS, "pairs": a.pairs, "threads": a.threads, "bam_bytes": os.path.getsize(bam), "regions": a.regions, "runs": runs},
                      open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""FASTQ files to the three extraction files: extract-sequence's host walk against --gpu-select (profiles/r15_gpu_select.json).

The sample is tools/bam_inflate_f2f.py's: the first PAIRS pairs of the C4 workload (tools/gen_synth.py) as plain FASTQ in memory-backed storage, mapped with
-ax sr --sorted-bam -l 5; the rows are `extract-reads --noprune` over that BAM and a BED of --regions regions of 20 kb spread evenly over the reference.
`extract-sequence` then runs in five forms: the parent commit's build (--parent DIR: the directory that holds its bin/ and lib/) on the plain files, this tree with
--gpu-select on the plain files, the parent's build on the same files as BGZF (gzread), this tree with --gpu-select --gpu-inflate on the same files as BGZF (0xff00-byte blocks, zlib level 6), and this tree with --gpu-select=host
(the kernels' host twin behind the same driver).  One warm-up round that is recorded as rep 0 and not reported, then --reps rounds, the forms alternating.
Per run: wall seconds of the process, the pieces of the two AL_TIMING lines (summed over the two files), and the md5 of the three output files, which must be
equal in every run.  Every process runs under a time limit; the series stops at the first run that fails.

    python tools/select_f2f.py --parent /path/to/parent/airlift_amd --out profiles/r15_gpu_select.json
"""
import argparse
import hashlib
import json
import multiprocessing
import os
import re
import struct
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

FIELDS = ("wall_s = the process, start to exit; the rest is summed over the two files' AL_TIMING lines: file_read_s = pread of the pieces; copy_up_s, kernel_s, copy_down_s = HIP events "
          "around the copies up (BGZF: the inflate launches included), the index / parse / select / scan / gather kernels and the copies down; select_wall_s = the selector's calls; "
          "tested, selected, handed = records; rep 0 is the warm-up round and is not reported")
EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def _member(block):
    c = zlib.compressobj(6, zlib.DEFLATED, -15); raw = c.compress(block) + c.flush()
    return struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 0x42, 0x43, 2, len(raw) + 25) + raw + struct.pack("<II", zlib.crc32(block), len(block))


def bgzf_file(src, dst, procs):
    with open(src, "rb") as f, open(dst, "wb") as o, multiprocessing.Pool(procs) as pool:
        while True:
            data = f.read(64 * 0xff00 * procs)
            if not data:
                break
            for m in pool.imap(_member, [data[i:i + 0xff00] for i in range(0, len(data), 0xff00)], chunksize=16):
                o.write(m)
        o.write(EOF_BLOCK)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="airlift_amd directory of the parent commit's build (bin/airlift-align, lib/libairlift.so)")
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--regions", type=int, default=300)
    ap.add_argument("--dir", default="/dev/shm/al_r15")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_gpu_select.json"))
    ap.add_argument("--limit", type=int, default=180, help="seconds a run may take")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    this = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
    ref_fa, f1, f2, bam, bed, rows = (os.path.join(a.dir, n) for n in ("ref.fa", "r_1.fq", "r_2.fq", "reads.bam", "regions.bed", "rows.bed"))
    t0 = time.time()
    if not all(os.path.exists(p) for p in (ref_fa, f1, f2)):
        import gen_synth as g
        sys.path.insert(0, ROOT)
        import bench                                               # the workload is bench.py's: same fragments, same names
        ref = g.build_reference("c4"); g.write_fasta(ref_fa, ref); print("reference written at %.0f s" % (time.time() - t0), flush=True)
        arr = bench.make_workload("c4", 0, a.pairs, 150, 20261002, ref)
        bench.write_fastq_fast(f1, arr, 0); bench.write_fastq_fast(f2, arr, 1)
        del ref, arr
        print("workload written at %.0f s" % (time.time() - t0), flush=True)
    if not os.path.exists(bam):
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), this, "-ax", "sr", "-t", str(a.threads), "--sorted-bam", "-l", "5", "-o", bam, ref_fa, f1, f2], stderr=subprocess.PIPE, env=dict(os.environ, AL_PG_PLAIN="1"))
        if r.returncode != 0:
            print("the mapping run failed (%d)\n%s" % (r.returncode, r.stderr.decode(errors="replace")[-3000:]), flush=True)
            return 1
        print("BAM written at %.0f s" % (time.time() - t0), flush=True)
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
    if not os.path.exists(rows):
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), this, "extract-reads", "--noprune", bam, bed], stdout=open(rows, "wb"), stderr=subprocess.PIPE)
        if r.returncode != 0:
            print("extract-reads failed (%d)\n%s" % (r.returncode, r.stderr.decode(errors="replace")[-3000:]), flush=True)
            return 1
    z1, z2 = f1 + ".gz", f2 + ".gz"
    for s, d in ((f1, z1), (f2, z2)):
        if not os.path.exists(d):
            bgzf_file(s, d, a.threads)
            print("%s written at %.0f s" % (os.path.basename(d), time.time() - t0), flush=True)
    trees = {"parent": os.path.join(a.parent, "bin", "airlift-align"), "this": this}
    series = [("host_walk", "parent", [], (f1, f2)), ("gpu_select", "this", ["--gpu-select"], (f1, f2)), ("host_walk_bgzf", "parent", [], (z1, z2)),
              ("gpu_select_bgzf", "this", ["--gpu-select", "--gpu-inflate"], (z1, z2)), ("host_twin", "this", ["--gpu-select=host"], (f1, f2))]
    runs = []; md5_all = None
    outd = os.path.join(a.dir, "out"); os.makedirs(outd, exist_ok=True)
    for rep in range(a.reps + 1):
        for name, tree, opts, fq in series:
            cmd = ["timeout", "-k", "10", str(a.limit), trees[tree], "extract-sequence"] + opts + [fq[0], fq[1], rows, outd]
            t1 = time.time()
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, AL_TIMING="1"))
            wall = time.time() - t1
            err = r.stderr.decode(errors="replace")
            if r.returncode != 0:
                print("run failed (%d): %s\n%s" % (r.returncode, " ".join(cmd), err[-3000:]), flush=True)
                json.dump({"failed": cmd, "rc": r.returncode, "runs": runs}, open(a.out, "w"), indent=1)
                return 1
            md5 = [hashlib.md5(open(os.path.join(outd, f), "rb").read()).hexdigest() for f in ("reads_1.fastq", "reads_2.fastq", "singletons.fastq")]
            tot = lambda rx, cast=float: (lambda v: round(sum(cast(x) for x in v), 4) if v else None)(re.findall(rx, err))
            rec = dict(rep=rep, form=name, tree=tree, wall_s=round(wall, 3), md5=md5, backend=(re.findall(r"--gpu-select '[^']*' \(([^)]*)\)", err) or [None])[0],
                       pieces=tot(r"(\d+) pieces,", int), bytes_in=tot(r"(\d+) bytes in,", int), tested=tot(r"(\d+) records tested", int), selected=tot(r"(\d+) selected", int),
                       handed=tot(r"(\d+) handed", int), file_read_s=tot(r"file read ([0-9.]+) s"), copy_up_s=tot(r"copy up ([0-9.]+) s"), kernel_s=tot(r"kernels ([0-9.]+) s"),
                       copy_down_s=tot(r"copy down ([0-9.]+) s"), select_wall_s=tot(r"wall ([0-9.]+) s"), pairs=(re.findall(r"(\d+) pairs, (\d+) singletons", err) or [None])[0])
            if md5_all is None:
                md5_all = md5
            rec["md5_equal"] = md5 == md5_all
            runs.append(rec)
            print(json.dumps(rec), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump({"what": __doc__.strip().split("\n\n")[1], "fields": FIELDS, "pairs": a.pairs, "fastq_bytes": [os.path.getsize(f1), os.path.getsize(f2)], "bgzf_bytes": [os.path.getsize(z1), os.path.getsize(z2)],
                       "rows": sum(1 for _ in open(rows)), "regions": a.regions, "runs": runs}, open(a.out, "w"), indent=1)
            if not rec["md5_equal"]:
                print("the output differs from the first run's", flush=True)
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())

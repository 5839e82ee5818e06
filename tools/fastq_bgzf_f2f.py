#!/usr/bin/env python3
"""FASTQ file to SAM file with BGZF-compressed reads: the host reader against --gpu-inflate of the mapping commands (DESIGN.md section 5,
profiles/r14_fastq_bgzf.json).

The input is the first PAIRS pairs of the C4 workload (tools/gen_synth.py, bench.py), as plain FASTQ and as BGZF made here with Python zlib (blocks of
0xff00 bytes, level 6, an EOF block), in memory-backed storage.  `airlift-align -ax sr` then runs in three forms, all from this tree: (a) the plain files;
(b) the BGZF files without the flag (the host driver's gzread + kseq reader: what the parent commit does with this input); (c) the BGZF files with
--gpu-inflate.  One warm-up round that is recorded as rep 0 and not reported,
then --reps rounds, the forms alternating.  Per run: wall seconds, the AL_TIMING parts of the stream pipeline and of its BGZF input, and the md5 of the
SAM, which must be equal in every run.
Every process runs under a time limit; the series stops at the first run that fails.

    python tools/fastq_bgzf_f2f.py --out profiles/r14_fastq_bgzf.json
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

FIELDS = ("wall_s = the process, start to exit; pipeline_s, reads_per_s_M, load_s, parse_s = total, rate, ingest load and parse+carry of the stream pipeline's AL_TIMING line (absent in "
          "form b, which takes the host driver); members, launches, bytes_in, bytes_out, kernel_s = the line's BGZF part (kernel_s: HIP events around the inflate kernels, summed); "
          "kernel_GBps_out = bytes_out / kernel_s; rep 0 is the warm-up round and is not reported")
EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
BLOCK = 0xff00


def member(chunk):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = c.compress(chunk) + c.flush()
    total = 18 + len(raw) + 8
    assert total <= 65536
    return b"\x1f\x8b\x08\x04" + bytes(4) + b"\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", total - 1) + raw + struct.pack("<II", zlib.crc32(chunk), len(chunk))


def span(args):
    path, lo, hi = args
    with open(path, "rb") as f:
        f.seek(lo); data = f.read(hi - lo)
    return b"".join(member(data[o:o + BLOCK]) for o in range(0, len(data), BLOCK))


def make_bgzf(src, dst, procs):
    size = os.path.getsize(src); step = BLOCK * 256
    with multiprocessing.Pool(procs) as pool, open(dst, "wb") as out:
        for part in pool.imap(span, [(src, lo, min(size, lo + step)) for lo in range(0, size, step)]):
            out.write(part)
        out.write(EOF_BLOCK)


def first(rx, text, cast=float):
    m = re.search(rx, text)
    return cast(m.group(1)) if m else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--dir", default="/dev/shm/al_r14")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_fastq_bgzf.json"))
    ap.add_argument("--limit", type=int, default=120, help="seconds a run may take")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    cli = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
    ref_fa, f1, f2, z1, z2, sam = (os.path.join(a.dir, n) for n in ("ref.fa", "r_1.fq", "r_2.fq", "r_1.fq.gz", "r_2.fq.gz", "out.sam"))
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
    for src, dst in ((f1, z1), (f2, z2)):
        if not os.path.exists(dst):
            make_bgzf(src, dst, a.threads)
    print("BGZF files written at %.0f s: %d + %d bytes of %d + %d" % (time.time() - t0, os.path.getsize(z1), os.path.getsize(z2), os.path.getsize(f1), os.path.getsize(f2)), flush=True)
    series = [("a_plain", [], [f1, f2], {}), ("b_bgzf_host_reader", [], [z1, z2], {}), ("c_bgzf_gpu_inflate", ["--gpu-inflate"], [z1, z2], {})]
    runs = []
    for rep in range(a.reps + 1):
        for name, opts, files, env in series:
            cmd = ["timeout", "-k", "10", str(a.limit), cli, "-ax", "sr", "-t", str(a.threads)] + opts + ["-o", sam, ref_fa] + files
            t1 = time.time()
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, AL_TIMING="1", AL_PG_PLAIN="1", **env))
            wall = time.time() - t1
            err = r.stderr.decode(errors="replace")
            if r.returncode != 0:
                print("run failed (%d): %s\n%s" % (r.returncode, " ".join(cmd), err[-3000:]), flush=True)
                json.dump({"failed": cmd, "rc": r.returncode, "runs": runs}, open(a.out, "w"), indent=1)
                return 1
            h = hashlib.md5()
            with open(sam, "rb") as f:
                for blk in iter(lambda: f.read(1 << 24), b""):
                    h.update(blk)
            rec = dict(rep=rep, form=name, wall_s=round(wall, 3), sam_bytes=os.path.getsize(sam), md5=h.hexdigest(),
                       pipeline_s=first(r"stream pipeline: .* in ([0-9.]+) s \(", err), reads_per_s_M=first(r"\(([0-9.]+) M reads/s\)", err),
                       load_s=first(r"ingest: wait-slot [0-9.]+ load ([0-9.]+)", err), parse_s=first(r"parse\+carry ([0-9.]+)", err),
                       members=first(r"BGZF input \([^)]*\): ([0-9]+) members", err, int), launches=first(r"members in ([0-9]+) launches", err, int),
                       bytes_in=first(r"launches, ([0-9]+) bytes in", err, int), bytes_out=first(r"bytes in, ([0-9]+) bytes out", err, int), kernel_s=first(r"bytes out, kernels ([0-9.]+) s", err))
            if rec["kernel_s"]:
                rec["kernel_GBps_out"] = round(rec["bytes_out"] / rec["kernel_s"] / 1e9, 2)
            runs.append(rec)
            print(json.dumps(rec), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump({"what": __doc__.strip().split("\n\n")[1], "fields": FIELDS, "pairs": a.pairs, "threads": a.threads,
                       "bytes": {"plain": [os.path.getsize(f1), os.path.getsize(f2)], "bgzf": [os.path.getsize(z1), os.path.getsize(z2)]}, "runs": runs}, open(a.out, "w"), indent=1)
    os.remove(sam)
    return 0 if len({r["md5"] for r in runs}) == 1 else 2


if __name__ == "__main__":
    sys.exit(main())

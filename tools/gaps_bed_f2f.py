#!/usr/bin/env python3
"""Gap regions to merged regions: `tokens ... REF.fa GAPS.fa` against `tokens --gaps-bed GAPS.bed ... REF.fa` (profiles/r18_gaps_bed.json).

The input is that of tools/regions_f2f.py: the yeast-sized C2 reference of tools/gen_synth.py and --windows windows of --window-len bases at even distances;
--read-size 150 --skip 1 makes about 9.7 M tokens of 2 000 windows of 5 kb.  The same windows are written as a gaps BED and as the GAPS.fa cut from it
(tests/tokens_cases.py: what `samtools faidx` prints per row).  Two forms alternate on one box, both with --regions-bed --merged-bed: (a) the parent commit's
build (--parent DIR: the directory that holds its bin/ and lib/) over REF.fa GAPS.fa -- the FASTA is made beforehand and not timed, which favours (a): the
flow it stands for also runs one `samtools faidx` process per row --, and (b) this tree with --gaps-bed.  One warm-up round that is recorded as rep 0 and not
reported, then --reps rounds.  Per run: wall seconds of the process, the md5 of both BED files, which must be equal across forms and runs, and the AL_TIMING
lines.  Verdict by the rule of DESIGN.md section 5: (b) is faster only if the smallest gap between the forms exceeds the largest difference between two runs
of one form.

    python tools/gaps_bed_f2f.py --parent /path/to/parent/airlift_amd --out profiles/r18_gaps_bed.json
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

FIELDS = ("wall_s = the process, start to exit; md5 = of the per-gap and the merged BED file; timing = the process's AL_TIMING lines that name the index build, the regions "
          "and, in (b), the token set-up (k_tok_setup_ms = HIP events summed over the run); rep 0 is the warm-up round and is not reported")


def md5(path):
    h = hashlib.md5()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="airlift_amd directory of the parent commit's build (bin/airlift-align, lib/libairlift.so)")
    ap.add_argument("--windows", type=int, default=2000)
    ap.add_argument("--window-len", type=int, default=5000)
    ap.add_argument("--read-size", type=int, default=150)
    ap.add_argument("--skip", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--dir", default="/dev/shm/al_r18")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_gaps_bed.json"))
    ap.add_argument("--limit", type=int, default=240, help="seconds a run may take")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    ref_fa, gaps_fa, gaps_bed = (os.path.join(a.dir, n) for n in ("ref.fa", "gaps.fa", "gaps.bed"))
    import gen_synth as g
    import tokens_cases as tc
    ref = g.build_reference("c2"); g.write_fasta(ref_fa, ref)
    tr = bytes.maketrans(bytes(range(5)), b"ACGTN"); rows = []
    total = sum(len(c) for _, c in ref); step = total // a.windows
    for k in range(a.windows):
        at = k * step
        for name, c in ref:
            if at < len(c):
                at = min(at, len(c) - a.window_len)
                rows.append(tc.row(name.encode() if isinstance(name, str) else name, at, a.window_len))
                break
            at -= len(c)
    bed = b"\n".join(rows) + b"\n"
    open(gaps_bed, "wb").write(bed)
    seqs = [(n.encode() if isinstance(n, str) else n, c.tobytes().translate(tr).decode()) for n, c in ref]
    open(gaps_fa, "wb").write(tc.gaps_fasta(bed, seqs))
    n_tokens = a.windows * len(range(a.read_size, a.window_len, a.skip))
    del ref, seqs
    tok = ["tokens", "--read-size", str(a.read_size), "--skip", str(a.skip), "-t", str(a.threads)]
    forms = [("a_fasta", os.path.join(a.parent, "bin", "airlift-align"), [], [ref_fa, gaps_fa]), ("b_gaps_bed", os.path.join(ROOT, "airlift_amd", "bin", "airlift-align"), ["--gaps-bed", gaps_bed], [ref_fa])]
    runs = []; first = []; extra = {}
    doc = lambda: {"what": __doc__.strip().split("\n\n")[1], "fields": FIELDS, "windows": a.windows, "window_len": a.window_len, "read_size": a.read_size, "skip": a.skip, "tokens": n_tokens,
                   "bed_bytes": len(bed), "gaps_fa_bytes": os.path.getsize(gaps_fa), "runs": runs, **extra}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for rep in range(a.reps + 1):
        for name, exe, opts, files in forms:
            outs = [os.path.join(a.dir, name + "_regions.bed"), os.path.join(a.dir, name + "_merged.bed")]
            cmd = ["timeout", "-k", "10", str(a.limit), exe] + tok + opts + ["--regions-bed", outs[0], "--merged-bed", outs[1]] + files
            t1 = time.time()
            r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=dict(os.environ, AL_TIMING="1", AL_PG_PLAIN="1"))
            wall = time.time() - t1
            err = r.stderr.decode(errors="replace")
            if r.returncode != 0:
                print("run failed (%d): %s\n%s" % (r.returncode, " ".join(cmd), err[-3000:]), flush=True)
                json.dump(dict(doc(), failed=cmd, rc=r.returncode), open(a.out, "w"), indent=1)
                return 1
            rec = dict(rep=rep, form=name, wall_s=round(wall, 3), md5=[md5(p) for p in outs], out_bytes=[os.path.getsize(p) for p in outs],
                       timing=[l for l in err.split("\n") if re.search(r"index build|regions:|tokens --gaps-bed", l)])
            m = re.search(r"k_tok_setup ([0-9.]+) ms", err)
            if m:
                rec["k_tok_setup_ms"] = float(m.group(1))
            first = first or rec["md5"]
            rec["md5_equal"] = rec["md5"] == first
            runs.append(rec); print(json.dumps(rec), flush=True)
            json.dump(doc(), open(a.out, "w"), indent=1)
            if not rec["md5_equal"]:
                print("the BED files differ from the first run's", flush=True)
                return 1
    wa = [r["wall_s"] for r in runs if r["rep"] and r["form"] == "a_fasta"]; wb = [r["wall_s"] for r in runs if r["rep"] and r["form"] == "b_gaps_bed"]
    spread = max(max(wa) - min(wa), max(wb) - min(wb)); gap = min(wa) - max(wb)
    extra.update(a_wall_s=wa, b_wall_s=wb, smallest_gap_s=round(gap, 3), largest_spread_s=round(spread, 3),
                 verdict="(b) is faster than (a)" if gap > spread else "(a) is faster than (b)" if max(wa) - min(wb) < -spread else "no difference beyond the run-to-run spread")
    json.dump(doc(), open(a.out, "w"), indent=1)
    print(extra["verdict"], extra, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

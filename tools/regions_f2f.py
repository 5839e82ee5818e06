#!/usr/bin/env python3
"""Gap sequences to merged regions: `tokens` writing SAM against `tokens --regions-bed --merged-bed` (profiles/r16_regions.json).

The input is the yeast-sized C2 reference of tools/gen_synth.py and a GAPS.fa of --windows windows of --window-len bases cut from it at even distances;
--read-size 150 --skip 1 makes about 9.7 M tokens of 2 000 windows of 5 kb.  Two forms alternate on one box: (a) the parent commit's build (--parent DIR: the
directory that holds its bin/ and lib/), `tokens ... > x.sam` in memory-backed storage, and (b) this tree, `tokens --regions-bed --merged-bed`.  One warm-up
round that is recorded as rep 0 and not reported, then --reps rounds.  Per run: wall seconds of the process and the md5 of its outputs, which must be equal in
every run of a form.  (a') = (a) plus the plain Python restatement of sort-bed | mergeBed over its SAM (tests/regions_cases.py), timed once: a stand-in for
`samtools view -F4 | samtools sort | convert2bed | mergeBed ...`, which are not at hand -- the real tools are compiled and would be faster than the
restatement, so (a) < real flow < (a').  The restatement's BED files must equal (b)'s.  Verdict by the rule of DESIGN.md section 5: (b) is faster only if the
smallest gap between the forms exceeds the largest difference between two runs of one form.

    python tools/regions_f2f.py --parent /path/to/parent/airlift_amd --out profiles/r16_regions.json
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

FIELDS = ("wall_s = the process, start to exit; md5 = of x.sam (a) or of the two BED files (b); (b) only, from its AL_TIMING line: intervals = records turned into "
          "intervals, folds, k_reg_intervals_ms and folds_ms = HIP events summed over the run, h2d_bytes / d2h_bytes = what the regions code copied; "
          "d2h_bytes_records (a) = 12 bytes per token + 112 per record, the result block al_fetch_raw copies without its CIGAR arena (computed, not counted); "
          "rep 0 is the warm-up round and is not reported")


def md5(path):
    h = hashlib.md5()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def restate(sam_path, gap_names):
    """the restatement over a SAM file, streamed: (per-gap BED, merged BED, records, mapped records)"""
    import regions_cases as rc
    gidx = {n: i for i, n in enumerate(gap_names)}; names = []; v = []; n_rec = 0
    span = re.compile(rb"(\d+)[MDN=X]")
    with open(sam_path, "rb") as f:
        for line in f:
            if line[:1] == b"@":
                if line.startswith(b"@SQ"):
                    names.append(line.split(b"\t")[1][3:])
                continue
            q = line.split(b"\t", 6); n_rec += 1
            if int(q[1]) & 4:
                continue
            s = int(q[3]) - 1
            v.append((gidx[q[0].rsplit(b"_", 1)[0]], names.index(q[2]), s, s + sum(map(int, span.findall(q[5])))))
    return rc.bed(rc.merge(v, names, True), names), rc.bed(rc.merge(v, names, False), names), n_rec, len(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="airlift_amd directory of the parent commit's build (bin/airlift-align, lib/libairlift.so)")
    ap.add_argument("--windows", type=int, default=2000)
    ap.add_argument("--window-len", type=int, default=5000)
    ap.add_argument("--read-size", type=int, default=150)
    ap.add_argument("--skip", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--dir", default="/dev/shm/al_r16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_regions.json"))
    ap.add_argument("--limit", type=int, default=240, help="seconds a run may take")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    ref_fa, gaps_fa, sam, bed_r, bed_m = (os.path.join(a.dir, n) for n in ("ref.fa", "gaps.fa", "x.sam", "regions.bed", "merged.bed"))
    import gen_synth as g
    ref = g.build_reference("c2"); g.write_fasta(ref_fa, ref)
    tr = bytes.maketrans(bytes(range(5)), b"ACGTN"); gap_names = []
    total = sum(len(c) for _, c in ref); step = total // a.windows
    with open(gaps_fa, "wb") as f:
        for k in range(a.windows):
            at = k * step
            for name, c in ref:
                if at < len(c):
                    at = min(at, len(c) - a.window_len)
                    nm = ("%s:%d-%d" % (name, at, at + a.window_len)).encode(); gap_names.append(nm)
                    f.write(b">" + nm + b"\n" + c[at:at + a.window_len].tobytes().translate(tr) + b"\n")
                    break
                at -= len(c)
    n_tokens = a.windows * len(range(a.read_size, a.window_len, a.skip))
    del ref
    tok = ["tokens", "--read-size", str(a.read_size), "--skip", str(a.skip), "-t", str(a.threads)]
    forms = [("a_sam", os.path.join(a.parent, "bin", "airlift-align"), [], [sam]), ("b_regions", os.path.join(ROOT, "airlift_amd", "bin", "airlift-align"), ["--regions-bed", bed_r, "--merged-bed", bed_m], [bed_r, bed_m])]
    runs = []; first = {}; extra = {}
    doc = lambda: {"what": __doc__.strip().split("\n\n")[1], "fields": FIELDS, "windows": a.windows, "window_len": a.window_len, "read_size": a.read_size, "skip": a.skip, "tokens": n_tokens,
                   "runs": runs, **extra}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for rep in range(a.reps + 1):
        for name, exe, opts, outs in forms:
            cmd = ["timeout", "-k", "10", str(a.limit), exe] + tok + opts + [ref_fa, gaps_fa]
            t1 = time.time()
            with open(sam if name == "a_sam" else os.devnull, "wb") as so:
                r = subprocess.run(cmd, stdout=so, stderr=subprocess.PIPE, env=dict(os.environ, AL_TIMING="1", AL_PG_PLAIN="1"))
            wall = time.time() - t1
            err = r.stderr.decode(errors="replace")
            if r.returncode != 0:
                print("run failed (%d): %s\n%s" % (r.returncode, " ".join(cmd), err[-3000:]), flush=True)
                json.dump(dict(doc(), failed=cmd, rc=r.returncode), open(a.out, "w"), indent=1)
                return 1
            rec = dict(rep=rep, form=name, wall_s=round(wall, 3), md5=[md5(p) for p in outs], out_bytes=[os.path.getsize(p) for p in outs])
            m = re.search(r"regions: (\d+) intervals, (\d+) folds, (\d+) per-gap regions, (\d+) merged; k_reg_intervals ([0-9.]+) ms, folds ([0-9.]+) ms; bytes to the device (\d+), from the device (\d+)", err)
            if m:
                rec.update(intervals=int(m.group(1)), folds=int(m.group(2)), per_gap_regions=int(m.group(3)), merged_regions=int(m.group(4)), k_reg_intervals_ms=float(m.group(5)),
                           folds_ms=float(m.group(6)), h2d_bytes=int(m.group(7)), d2h_bytes=int(m.group(8)))
            rec["md5_equal"] = rec["md5"] == first.setdefault(name, rec["md5"])
            runs.append(rec); print(json.dumps(rec), flush=True)
            json.dump(doc(), open(a.out, "w"), indent=1)
            if not rec["md5_equal"]:
                print("the output differs from the form's first run", flush=True)
                return 1
            if name == "b_regions" and rep == 1:     # (a') once, over the SAM form (a) has just written; its BED files against (b)'s
                t1 = time.time(); pg, al, n_rec, n_map = restate(sam, gap_names); t_re = time.time() - t1
                same = pg == open(bed_r, "rb").read() and al == open(bed_m, "rb").read()
                extra.update(restatement_s=round(t_re, 3), restatement_equals_b=same, sam_records=n_rec, sam_mapped_records=n_map, d2h_bytes_records=12 * n_tokens + 112 * n_map)
                print("restatement %.1f s over %d records (%d mapped): %s (b)'s files" % (t_re, n_rec, n_map, "equals" if same else "DIFFERS FROM"), flush=True)
                json.dump(doc(), open(a.out, "w"), indent=1)
                if not same:
                    return 1
    wa = [r["wall_s"] for r in runs if r["rep"] and r["form"] == "a_sam"]; wb = [r["wall_s"] for r in runs if r["rep"] and r["form"] == "b_regions"]
    spread = max(max(wa) - min(wa), max(wb) - min(wb)); gap = min(wa) - max(wb)
    extra.update(a_wall_s=wa, b_wall_s=wb, a_prime_wall_s=[round(x + extra.get("restatement_s", 0), 3) for x in wa], smallest_gap_s=round(gap, 3), largest_spread_s=round(spread, 3),
                 verdict="(b) is faster than (a)" if gap > spread else "(a) is faster than (b)" if max(wa) - min(wb) < -spread else "no difference beyond the run-to-run spread")
    json.dump(doc(), open(a.out, "w"), indent=1)
    print(extra["verdict"], extra, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Chain file to merged and retired regions: `tokens --gaps-bed GAPS.bed --merged-bed` of the parent build against `tokens --chain CHAIN --merged-bed
--retired-bed` of this tree, and the chainreg kernels against their host twin (profiles/r19_chain_beds.json).

The input is that of tools/regions_f2f.py and tools/gaps_bed_f2f.py: the yeast-sized C2 reference of tools/gen_synth.py and --windows windows of --window-len
bases at even distances; --read-size 150 --skip 1 makes about 9.7 M tokens of 2 000 windows of 5 kb.  The windows are written as a chain file, one chain per
contig, whose gaps rows (the gaps padded by read size + max errors) are those windows; a window that overlaps its predecessor (windows moved back from a
contig's end) is left out.  Two forms alternate on one box: (a) the parent commit's build (--parent DIR: the directory that holds its bin/ and lib/) with
--gaps-bed over the gaps BED `chain-beds --host --gaps-out` makes beforehand, not timed -- which favours (a): the flow it stands for also runs
2_get_updated_regions_bed.py before and get_retired_regions.py after --, writing --merged-bed; (b) this tree with --chain --max-errors, writing --merged-bed
and --retired-bed.  One warm-up round that is recorded as rep 0 and not reported, then --reps rounds.  Per run: wall seconds of the process, the md5 of every
output (merged equal across forms and runs, retired across runs and equal to `chain-beds --host --merged-in` over that merged BED), the AL_TIMING lines.
Required: (b) not slower than (a) by more than the largest difference between two runs of one form.

Device against twin: a synthetic chain file of --lines alignment lines over 24 contigs and a merged BED of --lines / 10 rows through `chain-beds` and
`chain-beds --host`, all three outputs, alternating, one warm-up and --reps runs: the HIP-event time of the device pass (first scan to last row copied back),
the wall time of the twin on the same table, and both processes' wall seconds.

    python tools/chain_beds_f2f.py --parent /path/to/parent/airlift_amd --out profiles/r19_chain_beds.json
"""
import argparse
import hashlib
import json
import os
import random
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")

FIELDS = ("wall_s = the process, start to exit; md5 = of every output file; timing = the process's AL_TIMING lines that name the index build, the regions, the token set-up and "
          "the chainreg passes (chainreg_ms = HIP events, per pass); rep 0 is the warm-up round and is not reported")


def md5(path):
    h = hashlib.md5()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def windows_chain(ref, n_windows, window_len, p):
    """(chain text, windows kept, windows left out): per contig one chain whose gaps, padded by p, are the windows [at + 1, at + window_len]"""
    total = sum(len(c) for _, c in ref); step = total // n_windows; per = {}
    for k in range(n_windows):
        at = k * step
        for name, c in ref:
            if at < len(c):
                per.setdefault(name, []).append(min(at, len(c) - window_len))
                break
            at -= len(c)
    out = []; kept = skipped = 0
    for cid, (name, c) in enumerate(ref, 1):
        name = name.decode() if isinstance(name, bytes) else name
        pos = 0; lines = []
        for at in sorted(per.get(name, [])):
            gs, ge = at + 1 + p, at + window_len - p                       # the raw gap, inclusive: the row is [gs - p, ge + p] = [at + 1, at + window_len]
            if gs <= pos or ge < gs:
                skipped += 1
                continue
            lines.append("%d %d 0" % (gs - pos, ge - gs + 1)); pos = ge + 1; kept += 1
        lines.append("%d" % (len(c) - pos))
        out.append("chain 1000 %s %d + 0 %d %s %d + 0 %d %d\n" % (name, len(c), len(c), name, len(c), len(c), cid) + "\n".join(lines) + "\n")
    return "\n".join(out), kept, skipped


def synthetic_chain(n_lines, seed=19):
    rnd = random.Random(seed); out = []; merged = []; n = 0; cid = 0
    L = 40 * 700 * (n_lines // 24 + 100)
    for c in range(24):
        pos = 0; want = n_lines // 24 + (1 if c < n_lines % 24 else 0); done = 0
        while done < want:
            k = min(rnd.randrange(1, 4000), want - done); start = pos + rnd.randrange(0, 500); cid += 1; at = start; lines = []
            for j in range(k):
                size = rnd.randrange(1, 700)
                if j + 1 == k:
                    lines.append("%d" % size); at += size
                else:
                    dt = rnd.choice([0, 0, 1, 2, rnd.randrange(0, 300), rnd.randrange(0, 40)]); lines.append("%d %d %d" % (size, dt, rnd.randrange(0, 50))); at += size + dt
            out.append("chain 1 s%d %d + %d %d q%d %d + 0 0 %d\n" % (c, L, start, at, c, L, cid) + "\n".join(lines) + "\n")
            pos = at; done += k
        assert pos < L
        for _ in range(n_lines // 240):
            s = rnd.randrange(0, L - 1); merged.append("s%d\t%d\t%d\n" % (c, s, s + rnd.randrange(0, 900)))
        n += done
    rnd.shuffle(merged)
    return "\n".join(out), "".join(merged), n


def run(cmd, limit, env=None):
    t1 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=dict(os.environ, AL_TIMING="1", AL_PG_PLAIN="1", **(env or {})))
    return r.returncode, time.time() - t1, r.stderr.decode(errors="replace")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="airlift_amd directory of the parent commit's build (bin/airlift-align, lib/libairlift.so)")
    ap.add_argument("--windows", type=int, default=2000)
    ap.add_argument("--window-len", type=int, default=5000)
    ap.add_argument("--read-size", type=int, default=150)
    ap.add_argument("--max-errors", type=int, default=5)
    ap.add_argument("--skip", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--lines", type=int, default=1000000)
    ap.add_argument("--dir", default="/dev/shm/al_r19")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_chain_beds.json"))
    ap.add_argument("--limit", type=int, default=240, help="seconds a run may take")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    P = lambda n: os.path.join(a.dir, n)
    import gen_synth as g
    ref = g.build_reference("c2"); g.write_fasta(P("ref.fa"), ref)
    chain, kept, skipped = windows_chain(ref, a.windows, a.window_len, a.read_size + a.max_errors)
    open(P("windows.chain"), "w").write(chain); chain_bytes = len(chain)
    del ref
    R, E = str(a.read_size), str(a.max_errors)
    rc, _, err = run([CLI, "chain-beds", "--host", "--read-size", R, "--max-errors", E, "--gaps-out", P("gaps.bed"), P("windows.chain")], a.limit)
    if rc != 0:
        print("chain-beds --host failed:", err[-2000:]); return 1
    n_rows = open(P("gaps.bed")).read().count("\n")
    n_tokens = n_rows * len(range(a.read_size, a.window_len, a.skip))
    runs = []; twin_runs = []; extra = {}
    doc = lambda: {"what": __doc__.strip().split("\n\n")[1], "fields": FIELDS, "windows": a.windows, "windows_kept": kept, "windows_left_out": skipped, "gaps_rows": n_rows, "window_len": a.window_len,
                   "read_size": a.read_size, "max_errors": a.max_errors, "skip": a.skip, "tokens": n_tokens, "chain_bytes": chain_bytes, "gaps_bed_bytes": os.path.getsize(P("gaps.bed")),
                   "runs": runs, "device_against_twin": twin_runs, **extra}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    save = lambda: json.dump(doc(), open(a.out, "w"), indent=1)
    tok = ["tokens", "--read-size", R, "--skip", str(a.skip), "-t", str(a.threads)]
    forms = [("a_gaps_bed", [os.path.join(a.parent, "bin", "airlift-align")] + tok + ["--gaps-bed", P("gaps.bed"), "--merged-bed", P("a_merged.bed"), P("ref.fa")], [P("a_merged.bed")]),
             ("b_chain", [CLI] + tok + ["--chain", P("windows.chain"), "--max-errors", E, "--merged-bed", P("b_merged.bed"), "--retired-bed", P("b_retired.bed"), P("ref.fa")], [P("b_merged.bed"), P("b_retired.bed")])]
    first = {}
    for rep in range(a.reps + 1):
        for name, cmd, outs in forms:
            rc, wall, err = run(cmd, a.limit)
            if rc != 0:
                print("run failed (%d): %s\n%s" % (rc, " ".join(cmd), err[-3000:]), flush=True)
                extra.update(failed=cmd, rc=rc); save()
                return 1
            rec = dict(rep=rep, form=name, wall_s=round(wall, 3), md5=[md5(p) for p in outs], out_bytes=[os.path.getsize(p) for p in outs],
                       timing=[l for l in err.split("\n") if re.search(r"index build|regions:|tokens --gaps-bed|tokens --chain|chainreg", l)],
                       chainreg_ms=[float(x) for x in re.findall(r"chainreg kernels ([0-9.]+) ms", err)])
            first.setdefault("merged", rec["md5"][0])
            if len(outs) > 1:
                first.setdefault("retired", rec["md5"][1])
            rec["md5_equal"] = rec["md5"][0] == first["merged"] and (len(outs) < 2 or rec["md5"][1] == first["retired"])
            runs.append(rec); print(json.dumps(rec), flush=True); save()
            if not rec["md5_equal"]:
                print("the BED files differ from the first run's", flush=True)
                return 1
    # the retired rows of (b) are the twin's over (b)'s merged BED
    rc, _, err = run([CLI, "chain-beds", "--host", "--read-size", R, "--merged-in", P("b_merged.bed"), "--retired-bed", P("twin_retired.bed"), P("windows.chain")], a.limit)
    extra["retired_equals_twin"] = rc == 0 and md5(P("twin_retired.bed")) == first["retired"]
    wa = [r["wall_s"] for r in runs if r["rep"] and r["form"] == "a_gaps_bed"]; wb = [r["wall_s"] for r in runs if r["rep"] and r["form"] == "b_chain"]
    spread = max(max(wa) - min(wa), max(wb) - min(wb))
    extra.update(a_wall_s=wa, b_wall_s=wb, largest_spread_s=round(spread, 3), b_slower_by_at_most_s=round(max(wb) - min(wa), 3),
                 verdict="(b) is faster than (a)" if min(wa) - max(wb) > spread else "(b) is slower than (a) by more than the run-to-run spread" if min(wb) - max(wa) > spread
                 else "no difference beyond the run-to-run spread")
    save()
    print(extra["verdict"], extra, flush=True)
    if not extra["retired_equals_twin"]:
        print("the retired rows differ from the twin's", flush=True)
        return 1
    # ---- device against twin --------------------------------------------------------------------------------------------------------------------------
    chain, merged, n_lines = synthetic_chain(a.lines)
    open(P("big.chain"), "w").write(chain); open(P("big_merged.bed"), "w").write(merged)
    extra.update(twin_lines=n_lines, twin_merged_rows=merged.count("\n"), twin_chain_bytes=len(chain))
    del chain, merged
    first = None
    for rep in range(a.reps + 1):
        for name, opt in (("device", []), ("twin", ["--host"])):
            outs = [P("%s_%s.bed" % (name, k)) for k in ("gaps", "constant", "retired")]
            rc, wall, err = run([CLI, "chain-beds"] + opt + ["--read-size", R, "--max-errors", E, "--gaps-out", outs[0], "--constant-bed", outs[1], "--merged-in", P("big_merged.bed"), "--retired-bed", outs[2], P("big.chain")], a.limit)
            if rc != 0:
                print("run failed (%d): chain-beds %s\n%s" % (rc, " ".join(opt), err[-3000:]), flush=True)
                extra.update(failed="chain-beds " + " ".join(opt), rc=rc); save()
                return 1
            m = re.search(r"(kernels|host twin) ([0-9.]+) ms", err)
            rec = dict(rep=rep, form=name, wall_s=round(wall, 3), function_ms=float(m.group(2)) if m else None, md5=[md5(p) for p in outs], rows=[open(p).read().count("\n") for p in outs],
                       timing=[l for l in err.split("\n") if "chainreg" in l])
            first = first or rec["md5"]; rec["md5_equal"] = rec["md5"] == first
            twin_runs.append(rec); print(json.dumps(rec), flush=True); save()
            if not rec["md5_equal"]:
                print("the BED files differ from the first run's", flush=True)
                return 1
    extra.update(device_ms=[r["function_ms"] for r in twin_runs if r["rep"] and r["form"] == "device"], twin_ms=[r["function_ms"] for r in twin_runs if r["rep"] and r["form"] == "twin"])
    save()
    print("device", extra["device_ms"], "twin", extra["twin_ms"], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

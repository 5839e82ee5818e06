#!/usr/bin/env python3
"""File-to-file timing of `chain-exact build` on the device and with --host (profiles/r22_chain_exact.json).

A synthetic pair is generated: --contigs contigs of --bases bases in all, the new reference a copy of the old one with substitutions at --rate, and one
chain per contig whose --blocks blocks are separated by gaps of 1 to 50 bases (dt = dq).  `chain-exact build` then runs on the device and with --host,
alternating, one warm-up round and --reps timed rounds; per run the wall time of the process, the md5 of the output (equal across forms and runs, or the
tool fails) and the process's AL_TIMING line: the FASTA load, the copies up, the kernels (HIP events: all, the fold, the count pass and the emit pass
alone), the device pass as the host sees it, pass 3 and the printing.  The compare kernels' rate is (bases compared x 2 sides) / time of the pass.

    python tools/chain_exact_f2f.py --out profiles/r22_chain_exact.json

For scale, --script PATH times the reference's run/1_build_exact_chain_file.py (with a stand-in `Bio` package, as tests/golden/make_g12_exact.py runs it) on
a cut of --script-bases bases of the same kind of pair and adds its bases per second to the JSON that is there; that part needs no GPU.
"""
import argparse
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "airlift_amd", "bin", "airlift-align")
FIELDS = ("wall_s = the process, start to exit; timing = the numbers of the process's AL_TIMING line in ms (kernels = HIP events around the whole device pass, fold / count / emit = "
          "the kernels of that name alone; device_pass = uploads, kernels and copies back as the host sees them); compare_GBps = 2 x bases / the count pass; "
          "round 0 is the warm-up and is not reported; median and min..max over the timed rounds")


def md5(path):
    h = hashlib.md5()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def write_fa(path, contigs, width=70):
    with open(path, "wb") as f:
        for name, a in contigs:
            f.write(b">" + name.encode() + b"\n")
            full = len(a) // width * width
            rows = np.empty((full // width, width + 1), dtype=np.uint8); rows[:, :width] = a[:full].reshape(-1, width); rows[:, width] = 10
            f.write(rows.tobytes())
            if full < len(a):
                f.write(a[full:].tobytes() + b"\n")


def make_pair(d, bases, n_contigs, n_blocks, rate, seed):
    """old.fa, new.fa, x.chain in d; (bases inside blocks, substitutions)"""
    rng = np.random.default_rng(seed); acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    old, new, chain, inside, n_sub = [], [], [], 0, 0
    for c in range(n_contigs):
        L = bases // n_contigs
        code = rng.integers(0, 4, L, dtype=np.uint8); a = acgt[code]
        k = max(1, int(L * rate)); at = rng.integers(0, L, k)
        b = a.copy(); b[at] = acgt[(code[at] + 1) % 4]; n_sub += len(np.unique(at))
        nb = max(1, n_blocks // n_contigs)
        gaps = rng.integers(1, 51, nb - 1); cuts = np.sort(rng.choice(np.arange(1, L - int(gaps.sum()) - 1), nb - 1, replace=False)) if nb > 1 else np.array([], dtype=np.int64)
        sizes = np.diff(np.concatenate(([0], cuts, [L - int(gaps.sum())])))
        assert (sizes > 0).all()
        lines = ["%d %d %d" % (s, g, g) for s, g in zip(sizes[:-1], gaps)] + ["%d" % sizes[-1]]
        inside += int(sizes.sum())
        chain.append("chain 1000 c%d %d + 0 %d c%d %d + 0 %d %d\n" % (c, L, L, c, L, L, c + 1) + "\n".join(lines) + "\n")
        old.append(("c%d" % c, a)); new.append(("c%d" % c, b))
    write_fa(os.path.join(d, "old.fa"), old); write_fa(os.path.join(d, "new.fa"), new)
    open(os.path.join(d, "x.chain"), "w").write("\n".join(chain))
    return inside, n_sub


def parse_timing(err):
    m = re.search(r"chainexact: .*", err)
    if not m:
        return {}
    l = m.group(0); out = {}
    for key, pat in (("blocks", r"(\d+) blocks"), ("bases", r"(\d+) bases"), ("mismatches", r"(\d+) mismatches"), ("lines", r"(\d+) lines"), ("load", r"load ([0-9.]+) ms"), ("h2d", r"to the device ([0-9.]+) ms"),
                     ("kernels", r"kernels ([0-9.]+) ms"), ("fold", r"fold ([0-9.]+)"), ("count", r"count ([0-9.]+)"), ("emit", r"emit ([0-9.]+)"), ("device_pass", r"device pass ([0-9.]+) ms"),
                     ("host_twin", r"host twin ([0-9.]+) ms"), ("text", r"text ([0-9.]+) ms")):
        g = re.search(pat, l)
        if g:
            out[key] = float(g.group(1)) if "." in g.group(1) else int(g.group(1))
    return out


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), n=len(v))


def time_script(script, d, bases, rate, seed):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_g12_exact as g12
    inside, _ = make_pair(d, bases, 2, 200, rate, seed)
    bio = tempfile.mkdtemp(prefix="al_r22_bio_"); os.makedirs(os.path.join(bio, "Bio"))
    open(os.path.join(bio, "Bio", "__init__.py"), "w").write(""); open(os.path.join(bio, "Bio", "SeqIO.py"), "w").write(g12.SEQIO)
    t = time.time()
    r = subprocess.run([sys.executable, script, "build", os.path.join(d, "old.fa"), os.path.join(d, "new.fa"), os.path.join(d, "x.chain")], env=dict(os.environ, PYTHONPATH=bio), capture_output=True)
    wall = time.time() - t
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    ours = subprocess.run([CLI, "chain-exact", "build", "--host", os.path.join(d, "old.fa"), os.path.join(d, "new.fa"), os.path.join(d, "x.chain")], capture_output=True)
    return dict(bases=inside, wall_s=wall, bases_per_s=inside / wall, same_bytes_as_host_twin=ours.returncode == 0 and ours.stdout == r.stdout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=1000000000)
    ap.add_argument("--contigs", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=100000)
    ap.add_argument("--rate", type=float, default=0.001)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=22)
    ap.add_argument("--dir", default="/dev/shm/al_r22")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_chain_exact.json"))
    ap.add_argument("--limit", type=int, default=240, help="seconds a run may take")
    ap.add_argument("--script", help="the reference's 1_build_exact_chain_file.py: time it alone on a cut of --script-bases, and add the figure to --out")
    ap.add_argument("--script-bases", type=int, default=2000000)
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    P = lambda n: os.path.join(a.dir, n)
    if a.script:
        res = json.load(open(a.out)) if os.path.exists(a.out) else {}
        res["reference_script"] = time_script(a.script, a.dir, a.script_bases, a.rate, a.seed)
        json.dump(res, open(a.out, "w"), indent=1, sort_keys=True)
        print(json.dumps(res["reference_script"]))
        return 0
    t = time.time()
    inside, n_sub = make_pair(a.dir, a.bases, a.contigs, a.blocks, a.rate, a.seed)
    res = dict(fields=FIELDS, args=vars(a), bases_in_blocks=inside, substitutions=n_sub, generate_s=time.time() - t, runs=[])
    print("generated %d bases in blocks, %d substitutions in %.1f s" % (inside, n_sub, res["generate_s"]), flush=True)
    want = None
    for rep in range(a.reps + 1):
        for form, opt in (("device", []), ("host", ["--host"])):
            out = P("out_%s.chain" % form)
            t1 = time.time()
            r = subprocess.run(["timeout", "-k", "10", str(a.limit), CLI, "chain-exact", "build"] + opt + ["-o", out, P("old.fa"), P("new.fa"), P("x.chain")], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                               env=dict(os.environ, AL_TIMING="1"))
            wall = time.time() - t1; err = r.stderr.decode(errors="replace")
            if r.returncode != 0:                                          # nothing more is started after a failed run
                print("run failed (%d): %s\n%s" % (r.returncode, form, err[-3000:]), flush=True)
                res.update(failed=form, rc=r.returncode); json.dump(res, open(a.out, "w"), indent=1, sort_keys=True)
                return 1
            h = md5(out); want = want or h
            if h != want:
                print("outputs differ: %s in round %d" % (form, rep)); return 1
            if rep:
                res["runs"].append(dict(form=form, rep=rep, wall_s=wall, md5=h, timing=parse_timing(err)))
            print(form, rep, "%.2f s" % wall, parse_timing(err), flush=True)
    summ = {}
    for form in ("device", "host"):
        runs = [x for x in res["runs"] if x["form"] == form]
        s = dict(wall_s=spread([x["wall_s"] for x in runs]))
        for k in ("load", "h2d", "kernels", "fold", "count", "emit", "device_pass", "host_twin", "text"):
            v = [x["timing"][k] for x in runs if k in x["timing"]]
            if v:
                s[k + "_ms"] = spread(v)
        if "count_ms" in s:
            s["compare_GBps"] = {k: 2 * inside / (s["count_ms"][m] * 1e-3) / 1e9 for k, m in (("median", "median"), ("best", "min"))}
        summ[form] = s
    res["summary"] = summ; res["output_md5"] = want; res["output_lines"] = sum(1 for _ in open(P("out_device.chain")))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(summ, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Golden SAM for the output options --MD, --cs[=long], --eqx, -Y: the bundled minimap2 fork compiled where it lies (map.c with the ALSER
early return removed, the same `sed '299,331d'` as oracle/Makefile) into a temp dir, driven by our own g8_tags_driver.c through the
public minimap.h API (the fork's main() prints counts instead of SAM, and oracle/_ref/mm2ref sets no output flags).  Authoring
container only (needs /root/reference); what is committed is data under g8_tags/: one SAM .gz per (input set, option set), the new
input set g8_chimeric (single-end chimeric reads with N runs, lower case and U on a two-contig reference) and meta.json.

    python tests/golden/make_g8_tags.py
"""
import glob, gzip, hashlib, json, os, shutil, subprocess, tempfile
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/src/minimap2-master_remapping"
OUT = os.path.join(HERE, "g8_tags")
SETS = ["g1_mt150pe", "g2_100se", "g2_250pe", "g3_adversarial", "g4_MT_orang", "g4_q_inv", "g6_repeats", "g8_chimeric"]
FLAGS = {"MD": ["--MD"], "cs": ["--cs"], "cs_long": ["--cs=long"], "MD_cs_long": ["--MD", "--cs=long"], "Y": ["-Y"], "Y_cs_long": ["-Y", "--cs=long"],
         "eqx": ["--eqx"], "Y_eqx_cs_long": ["-Y", "--eqx", "--cs=long"]}
# big paired sets take the MD tag (and -Y with long cs where they are not too large); the small and the new chimeric set every option set
PER_SET = {"g1_mt150pe": ["MD", "Y_cs_long"], "g2_250pe": ["MD"], "g3_adversarial": ["MD", "cs"],
           "g2_100se": ["MD", "cs", "MD_cs_long", "Y_cs_long", "eqx"], "g6_repeats": ["MD", "cs", "MD_cs_long", "Y_cs_long", "eqx"]}
REF_C = "kthread kalloc misc bseq sketch sdust options index chain align hit format pe esterr splitidx".split()


def build_fork(tmp):
    cc = ["gcc", "-c", "-O2", "-w", "-DHAVE_KALLOC", "-I" + REF]
    subprocess.run("sed '299,331d' %s/map.c > %s/map_ofull.c" % (REF, tmp), shell=True, check=True)
    for f in REF_C:
        subprocess.run(cc + [os.path.join(REF, f + ".c"), "-o", os.path.join(tmp, f + ".o")], check=True)
    subprocess.run(cc + [os.path.join(tmp, "map_ofull.c"), "-o", os.path.join(tmp, "map.o")], check=True)
    subprocess.run(cc + ["-msse2", os.path.join(REF, "ksw2_ll_sse.c"), "-o", os.path.join(tmp, "ksw2_ll_sse.o")], check=True)
    for f in ["extz2", "extd2", "exts2"]:
        subprocess.run(cc + ["-msse4.1", "-DKSW_CPU_DISPATCH", os.path.join(REF, "ksw2_%s_sse.c" % f), "-o", os.path.join(tmp, "ksw2_%s_sse41.o" % f)], check=True)
        subprocess.run(cc + ["-msse2", "-mno-sse4.1", "-DKSW_CPU_DISPATCH", "-DKSW_SSE2_ONLY", os.path.join(REF, "ksw2_%s_sse.c" % f), "-o", os.path.join(tmp, "ksw2_%s_sse2.o" % f)], check=True)
    subprocess.run(cc + ["-msse4.1", "-DKSW_CPU_DISPATCH", os.path.join(REF, "ksw2_dispatch.c"), "-o", os.path.join(tmp, "ksw2_dispatch.o")], check=True)
    subprocess.run(cc + [os.path.join(HERE, "g8_tags_driver.c"), "-o", os.path.join(tmp, "drv.o")], check=True)
    exe = os.path.join(tmp, "g8drv")
    subprocess.run(["gcc", "-O2", "-o", exe] + sorted(glob.glob(os.path.join(tmp, "*.o"))) + ["-lm", "-lz", "-lpthread"], check=True)
    return exe


COMP = str.maketrans("ACGTNacgtn", "TGCANtgcan")


def make_chimeric(d):
    """300 single-end reads of 150 bases: 80-100 bases from one contig joined to the rest from the other (or from far away on the
    same one), with substitutions, a short indel, N runs, lower case and U; half reverse-complemented."""
    rng = np.random.default_rng(8)
    ctg = ["".join("ACGT"[i] for i in rng.integers(0, 4, size=n)) for n in (30000, 22000)]
    with open(os.path.join(d, "chim.fa"), "w") as f:
        for i, s in enumerate(ctg):
            f.write(">ctg%d\n" % (i + 1))
            for o in range(0, len(s), 70):
                f.write(s[o:o + 70] + "\n")
    with open(os.path.join(d, "chim.fq"), "w") as f:
        for r in range(300):
            a = int(rng.integers(80, 101)); b = 150 - a
            c1 = int(rng.integers(0, 2)); c2 = 1 - c1 if r % 3 else c1
            p1 = int(rng.integers(0, len(ctg[c1]) - a)); p2 = int(rng.integers(0, len(ctg[c2]) - b))
            s = list(ctg[c1][p1:p1 + a] + ctg[c2][p2:p2 + b])
            for p in rng.integers(0, 150, size=int(rng.integers(0, 4))):
                s[int(p)] = "ACGT"[int(rng.integers(0, 4))]
            if r % 5 == 0:
                p = int(rng.integers(10, 60)); s[p:p + int(rng.integers(1, 6))] = "N" * int(rng.integers(1, 6))
            if r % 7 == 1:
                p = int(rng.integers(20, 120)); del s[p:p + int(rng.integers(1, 4))]
            if r % 7 == 3:
                p = int(rng.integers(20, 120)); s[p:p] = list("ACGT"[int(rng.integers(0, 4))] * int(rng.integers(1, 3)))
            t = "".join(s)
            if r % 2:
                t = t.translate(COMP)[::-1]
            if r % 4 == 1:
                t = "".join(c.lower() if j % 5 < 2 else c for j, c in enumerate(t))
            if r % 6 == 2:
                t = t.replace("T", "U", 3)
            f.write("@chim%d\n%s\n+\n%s\n" % (r, t, "".join(chr(33 + int(q)) for q in rng.integers(2, 41, size=len(t)))))


def main():
    tmp = tempfile.mkdtemp(prefix="al_g8_")
    try:
        exe = build_fork(tmp)
        shutil.rmtree(OUT, ignore_errors=True); os.makedirs(OUT)
        make_chimeric(tmp)
        for fn in ["chim.fa", "chim.fq"]:
            with gzip.GzipFile(os.path.join(OUT, fn + ".gz"), "wb", mtime=0) as f:
                f.write(open(os.path.join(tmp, fn), "rb").read())
        meta = {"flags": FLAGS, "sets": {}}
        for name in SETS:
            if name == "g8_chimeric":
                d, m = tmp, {"ref": "chim.fa", "reads": ["chim.fq"], "rg": None}
            else:
                src = os.path.join(HERE, name); d = os.path.join(tmp, name); os.makedirs(d)
                for fn in os.listdir(src):
                    if fn.endswith(".gz"):
                        open(os.path.join(d, fn[:-3]), "wb").write(gzip.open(os.path.join(src, fn)).read())
                m = json.load(open(os.path.join(src, "meta.json")))
            ent = {"ref": m["ref"], "reads": m["reads"], "rg": m.get("rg"), "out": {}}
            for key in PER_SET.get(name, list(FLAGS)):
                fl = FLAGS[key]
                cmd = [exe] + (["-R", m["rg"]] if m.get("rg") else []) + fl + [m["ref"]] + m["reads"]
                sam = subprocess.run(cmd, cwd=d, capture_output=True, check=True).stdout
                recs = [l.split(b"\t") for l in sam.split(b"\n") if l and not l.startswith(b"@")]
                with gzip.GzipFile(os.path.join(OUT, "%s__%s.sam.gz" % (name, key)), "wb", mtime=0) as f:
                    f.write(sam)
                ent["out"][key] = {"md5": hashlib.md5(sam).hexdigest(), "n_records": len(recs),
                                   "n_supplementary": sum(1 for r in recs if int(r[1]) & 0x800),
                                   "n_with_N": sum(1 for r in recs if b"N" in r[9].upper() and not int(r[1]) & 4),
                                   "n_gapped": sum(1 for r in recs if b"I" in r[5] or b"D" in r[5]),
                                   "n_MD": sum(1 for r in recs if any(x.startswith(b"MD:Z:") for x in r[11:])),
                                   "n_cs": sum(1 for r in recs if any(x.startswith(b"cs:Z:") for x in r[11:]))}
            meta["sets"][name] = ent
        json.dump(meta, open(os.path.join(OUT, "meta.json"), "w"), indent=1, sort_keys=True)
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()

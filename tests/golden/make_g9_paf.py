#!/usr/bin/env python3
"""Golden PAF (and --secondary=yes SAM) for --paf, -c, --cs, --paf-no-hit, --secondary: the bundled minimap2 fork compiled where it
lies (map.c with the ALSER early return removed, the same `sed '299,331d'` as oracle/Makefile) into a temp dir, driven by our own
g9_paf_driver.c through the public minimap.h API.  Authoring container only (needs /root/reference); what is committed is data under
g9_paf/: one .paf.gz / .sam.gz per (input set, option set) and meta.json (md5 and line counts per kind).  The inputs are the
existing golden sets; the chimeric reads are those of g8_tags/.

    python tests/golden/make_g9_paf.py
"""
import glob, gzip, hashlib, json, os, shutil, subprocess, tempfile
HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/src/minimap2-master_remapping"
OUT = os.path.join(HERE, "g9_paf")
# option set -> (driver / airlift-align options after the output format, file suffix)
FLAGS = {"paf": [], "c": ["-c"], "cs": ["--cs"], "MD": ["--MD"], "nohit": ["--paf-no-hit"], "sec": ["--secondary=yes"], "c_sec": ["-c", "--secondary=yes"],
         "c_eqx": ["-c", "--eqx"], "c_cs_long": ["-c", "--cs=long"], "c_Y": ["-c", "-Y"], "sam_sec": ["--secondary=yes"]}
PER_SET = {"g3_adversarial": ["paf", "c", "cs", "MD", "nohit", "sec", "c_sec", "sam_sec"], "g6_repeats": ["paf", "c", "sec", "c_sec", "sam_sec"],
           "g2_100se": ["paf", "c", "sec"], "g1_mt150pe": ["paf", "c"], "g8_chimeric": ["paf", "c_eqx", "c_cs_long", "c_Y"]}
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
    subprocess.run(cc + [os.path.join(HERE, "g9_paf_driver.c"), "-o", os.path.join(tmp, "drv.o")], check=True)
    exe = os.path.join(tmp, "g9drv")
    subprocess.run(["gcc", "-O2", "-o", exe] + sorted(glob.glob(os.path.join(tmp, "*.o"))) + ["-lm", "-lz", "-lpthread"], check=True)
    return exe


def counts(text, is_sam):
    lines = [l for l in text.split(b"\n") if l and not (is_sam and l.startswith(b"@"))]
    has = lambda l, t: (b"\t" + t) in l
    c = {"n_lines": len(lines), "n_tpS": sum(has(l, b"tp:A:S") for l in lines), "n_de": sum(has(l, b"de:f:") for l in lines),
         "n_cs": sum(has(l, b"cs:Z:") for l in lines), "n_MD": sum(has(l, b"MD:Z:") for l in lines)}
    if not is_sam:
        c["n_cg"] = sum(has(l, b"cg:Z:") for l in lines)
        c["n_no_hit"] = sum(l.split(b"\t")[4] == b"*" for l in lines)
    return c


def main():
    tmp = tempfile.mkdtemp(prefix="al_g9_")
    try:
        exe = build_fork(tmp)
        shutil.rmtree(OUT, ignore_errors=True); os.makedirs(OUT)
        meta = {"flags": FLAGS, "sets": {}}
        for name, keys in PER_SET.items():
            d = os.path.join(tmp, name); os.makedirs(d)
            if name == "g8_chimeric":
                for fn in ["chim.fa", "chim.fq"]:
                    open(os.path.join(d, fn), "wb").write(gzip.open(os.path.join(HERE, "g8_tags", fn + ".gz")).read())
                m = {"ref": "chim.fa", "reads": ["chim.fq"], "rg": None}
            else:
                src = os.path.join(HERE, name)
                for fn in os.listdir(src):
                    if fn.endswith(".gz"):
                        open(os.path.join(d, fn[:-3]), "wb").write(gzip.open(os.path.join(src, fn)).read())
                m = json.load(open(os.path.join(src, "meta.json")))
            ent = {"ref": m["ref"], "reads": m["reads"], "rg": m.get("rg"), "out": {}}
            for key in keys:
                is_sam = key.startswith("sam_")
                cmd = [exe] + (["-a"] if is_sam else []) + (["-R", m["rg"]] if m.get("rg") else []) + FLAGS[key] + [m["ref"]] + m["reads"]
                text = subprocess.run(cmd, cwd=d, capture_output=True, check=True).stdout
                fn = "%s__%s.%s.gz" % (name, key, "sam" if is_sam else "paf")
                if key == "MD":      # --MD without -c / --cs: no alignment, so no MD:Z (format.c:327 needs r->p) -- the bytes of the plain run, kept once
                    assert hashlib.md5(text).hexdigest() == ent["out"]["paf"]["md5"]
                    fn = ent["out"]["paf"]["file"]
                else:
                    with gzip.GzipFile(os.path.join(OUT, fn), "wb", mtime=0) as f:
                        f.write(text)
                ent["out"][key] = dict(counts(text, is_sam), md5=hashlib.md5(text).hexdigest(), file=fn)
            meta["sets"][name] = ent
        json.dump(meta, open(os.path.join(OUT, "meta.json"), "w"), indent=1, sort_keys=True)
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()

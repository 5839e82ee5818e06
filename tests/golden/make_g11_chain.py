#!/usr/bin/env python3
"""Golden vectors for `chain-beds` / `tokens --chain`: hand-made chain files through the reference's own three scripts -- 2_get_updated_regions_bed.py (the
gaps BED), get_constant_regions.py and get_retired_regions.py (with a hand-made merged BED).  Authoring container only (needs /root/reference); what is
committed is data: the chain files, the merged BEDs, the three outputs per case and meta.json (R, E, md5s).

    python tests/golden/make_g11_chain.py

Every chain file stays inside what both the scripts and the feature accept: '# ' comments, '+' strands, no name first seen as qName, every merged contig
named by a header, plain blank lines.  The cases:
  three    the three-chain file of DESIGN.md 7 (R 100, E 5): a dt = 0 line, a second chain on the first contig, merged rows on both contigs
  edges    dt = 0 with dq > 0; gaps within R + E of both contig ends; a contig shorter than R + E; comments and blank lines
  touch    two padded gaps with start == previous end (not merged: the strict rule); two padded blocks with start == previous end (merged) and with
           start == previous end + 1 (two regions, no hole); contigs covered from their first base and bare behind (the tail rule: no retired row)
  order    a merged contig that sorts before the chain's first contig and comes first in the merged BED (the retired slot order), interleaved tNames,
           a later header with a different tSize, two chains without a blank line between them, a merged row that ends beyond its contig
  random   1 900 alignment lines over five contigs, seeded
"""
import hashlib, json, os, random, subprocess, sys, tempfile
HERE = os.path.dirname(os.path.abspath(__file__))
GAPS_PY = "/root/reference/src/2-generate_gaps/2_get_updated_regions_bed.py"
CONST_PY = "/root/reference/src/4-extract_reads/get_constant_regions.py"
RETIRED_PY = "/root/reference/src/4-extract_reads/get_retired_regions.py"

THREE = """chain 1000 cA 5000 + 100 3900 qA 5000 + 100 3880 1
400 0 30
300 50 0
1000 200 200
1850

chain 900 cB 3000 + 0 3000 qB 3000 + 0 2990 2
1000 10 0
1990

chain 500 cA 5000 + 4200 4600 qA 5000 + 4100 4500 3
400
"""
EDGES = """# edge cases: gaps near both ends, an insertion (dt = 0), a contig shorter than the pad
chain 10 e1 1000 + 10 990 q1 1200 + 0 1000 1
20 5 0
100 0 7
800 15 3
40

# a contig of 40 bases

chain 5 tiny 40 + 0 40 q2 100 + 0 60 2
10 5 20
10 0 4
15
"""
TOUCH = """chain 1 t1 1000 + 0 181 u1 1000 + 0 169 1
100 10 0
19 2 0
50

chain 2 t2 2000 + 500 839 u2 2000 + 500 800 2
100 19 0
100 20 0
100

chain 3 t3 1000 + 0 300 u3 1000 + 0 300 3
300
"""
ORDER = """chain 1 zz 3000 + 100 600 qz 3000 + 0 510 1
200 50 10
250

chain 2 aa 2000 + 0 900 qa 2000 + 0 800 2
400 100 0
400

# the same contig again, with another tSize: the first one stays
chain 3 zz 2500 + 1000 1500 qz 3000 + 900 1400 3
100 30 30
370

chain 4 mm 800 + 100 700 qm 800 + 100 700 4
600
chain 5 aa 2000 + 1200 1900 qa 2000 + 1100 1800 5
300 100 100
300
"""


def random_case(seed=19, n_lines=1900):
    rnd = random.Random(seed)
    contigs = [("r%d" % i, rnd.randrange(150000, 400000)) for i in range(5)]
    at = [0] * 5; out = ["# %d alignment lines, seed %d" % (n_lines, seed)]; n = 0; cid = 0
    while n < n_lines:
        c = rnd.randrange(5); name, L = contigs[c]
        if L - at[c] < 3000:
            continue
        start = at[c] + rnd.randrange(0, 400); k = min(rnd.randrange(1, 60), n_lines - n); pos = start; lines = []
        for j in range(k):
            size = rnd.randrange(1, 700)
            dt = rnd.choice([0, 0, 1, 2, rnd.randrange(0, 300), rnd.randrange(0, 40)])
            last = j == k - 1 or pos + size + dt + 1500 > L
            if last:
                lines.append("%d" % size); pos += size
                break
            lines.append("%d %d %d" % (size, dt, rnd.randrange(0, 50))); pos += size + dt
        cid += 1; n += len(lines)
        out.append("chain %d %s %d + %d %d q%s %d + %d %d %d" % (rnd.randrange(1, 10 ** 6), name, L, start, pos, name, L + 1000, start, pos, cid))
        out += lines + [""]
        at[c] = pos + rnd.choice([0, 0, 50, 180, 260])
    merged = []
    for _ in range(150):
        name, L = contigs[rnd.randrange(4)]                                # (r4 has no merged row: its slot comes from the chain alone)
        s = rnd.randrange(0, L - 1); merged.append("%s\t%d\t%d" % (name, s, s + rnd.randrange(0, 900)))
    return "\n".join(out) + "\n", "\n".join(merged) + "\n"


RANDOM_CHAIN, RANDOM_MERGED = random_case()
CASES = [("three", THREE, 100, 5, "cA\t150\t900\ncA\t2500\t2600\ncB\t2000\t2050\n"),
         ("edges", EDGES, 50, 3, "e1\t200\t300\ntiny\t5\t8\n"),
         ("touch", TOUCH, 10, 0, "t2\t1200\t1300\n"),
         ("order", ORDER, 30, 2, "aa\t950\t1000\nmm\t0\t20\naa\t1950\t1990\nzz\t2900\t3400\n"),
         ("random", RANDOM_CHAIN, 150, 6, RANDOM_MERGED)]


def main():
    d = os.path.join(HERE, "g11_chain"); os.makedirs(d, exist_ok=True)
    meta = {}
    for name, chain, R, E, merged in CASES:
        tmp = tempfile.mkdtemp(prefix="al_g11_")
        cf = os.path.join(tmp, name + ".chain"); mf = os.path.join(tmp, name + ".merged.bed")
        open(cf, "w").write(chain); open(mf, "w").write(merged)
        outs = {k: os.path.join(tmp, "%s.%s.bed" % (name, k)) for k in ("gaps", "constant", "retired")}
        run = lambda *a: subprocess.run([sys.executable] + list(a), cwd=tmp, check=True, stdout=subprocess.DEVNULL)
        run(GAPS_PY, cf, str(R), str(E), outs["gaps"])
        run(CONST_PY, str(R), cf, outs["constant"])                        # (the script takes the file for a chain file by ".chain" in its name)
        run(RETIRED_PY, str(R), mf, cf, outs["retired"])
        m = {"read_size": R, "max_errors": E, "n_alignment_lines": sum(1 for l in chain.split("\n") if l and l[0].isdigit())}
        for f in [cf, mf] + list(outs.values()):
            data = open(f, "rb").read()
            open(os.path.join(d, os.path.basename(f)), "wb").write(data)
            m[os.path.basename(f)] = hashlib.md5(data).hexdigest()
        meta[name] = m
        print("g11_chain/%s: %d lines, %s rows" % (name, m["n_alignment_lines"], {k: open(v).read().count("\n") for k, v in outs.items()}))
    json.dump(meta, open(os.path.join(d, "meta.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()

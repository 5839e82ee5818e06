#!/usr/bin/env python3
"""Golden vectors for `chain-exact verify|build`: FASTA pairs and chain files through the reference's own run/1_build_exact_chain_file.py, both modes.
Authoring container only (needs /root/reference); what is committed is data: the FASTA pairs, the chain files, *.verify.txt, *.build.chain and meta.json
(md5 of every file).

    python tests/golden/make_g12_exact.py

The script imports Biopython, which the image lacks: a stand-in package `Bio` of our own is written to a temporary directory and put on PYTHONPATH --
SeqIO.parse is a FASTA reader that yields (first word of the header, sequence), SeqIO.to_dict is dict.  The script itself runs unmodified.  The cases:
  worked   the example of DESIGN.md 7: an insertion, nine substitutions, a head and a tail that move into the header
  minus    a '-' chain over a reverse-complemented contig with two substitutions (verify is silent for it: the block ends on the contig's last base)
  minus2   the same with bases to spare behind the blocks, so that verify compares them
  order    chains x->x, y->y, x->z and x->x at another tStart, in that file order: the output order differs
  ends     a mismatch at idx 0 and at the last idx of a block; a block that ends on the contig's last base (verify skips it); a 2-base chain; a chain that
           folds to its header alone; a 1-field last block under 100 bases, which is kept
  fold     good stretches of 99, 100 and 101 bases between mismatches; runs of adjacent mismatches; small blocks leading and trailing a chain
  letters  mixed case, N against n, R against R and against N on '+'
  random   five contigs of 100 000 to 300 000 bases, about 300 blocks, seeded substitutions at 0.1 %; its three input files (1.5 MB) are not committed:
           chainexact_cases.random_pair makes them again from numpy's frozen RandomState stream, and meta.json holds their md5
"""
import hashlib, json, os, random, subprocess, sys, tempfile
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import chainexact_cases as cx   # noqa: E402
SCRIPT = "/root/reference/run/1_build_exact_chain_file.py"
SEQIO = '''def parse(fn, fmt):
    name, seq = None, []
    for line in open(fn):
        if line.startswith(">"):
            if name is not None:
                yield name, "".join(seq)
            name, seq = line[1:].split()[0], []
        elif name is not None:
            seq.append(line.strip())
    if name is not None:
        yield name, "".join(seq)


to_dict = dict
'''


def rand_seq(rnd, n, alphabet="ACGT"):
    return "".join(rnd.choice(alphabet) for _ in range(n))


def sub(s, at):
    """s with another base at every position of `at`"""
    t = list(s)
    for k in at:
        t[k] = {"A": "C", "C": "G", "G": "T", "T": "A"}.get(t[k].upper(), "A")
    return "".join(t)


def worked(rnd):
    old = rand_seq(rnd, 2002)
    new = sub(old[:800] + "GGGGG" + old[800:] + "ACG", [0, 150, 151, 152, 799, 805, 1200, 1290, 2004])
    chain = "chain 5 x 2002 + 0 2000 x 2008 + 0 2005 1\n800 0 5\n1200\n"
    return [("x", old)], [("x", new)], chain


def minus(rnd):
    old = rand_seq(rnd, 1000)
    return [("m", old)], [("m", cx.revcomp(sub(old, [17, 998])))], "chain 9 m 1000 + 0 1000 m 1000 - 0 1000 3\n1000\n"


def minus2(rnd, spare=40):
    old = rand_seq(rnd, 1000 + spare)
    image = sub(old[:400], [17]) + rand_seq(rnd, 7) + sub(old[410:1000], [588])      # 400 10 7 / 590
    new = rand_seq(rnd, spare) + cx.revcomp(image)
    n = len(new)
    return [("m", old)], [("m", new)], "chain 9 m %d + 0 1000 m %d - 0 997 3\n400 10 7\n590\n" % (len(old), n)


def order(rnd):
    x, y = rand_seq(rnd, 3000), rand_seq(rnd, 1500)
    z = sub(x[1000:1600], [5, 300])
    new_x = sub(x, [100, 2500])
    chain = ("chain 1 x 3000 + 0 900 x 3000 + 0 900 1\n900\n\n"
             "chain 2 y 1500 + 100 1400 y 1500 + 100 1400 2\n600 50 50\n650\n\n"
             "chain 3 x 3000 + 1000 1600 z 600 + 0 600 3\n590\n\n"
             "chain 4 x 3000 + 2000 2900 x 3000 + 2000 2900 4\n400 100 100\n400\n")
    return [("x", x), ("y", y)], [("x", new_x), ("y", sub(y, [700])), ("z", z)], chain


def ends(rnd):
    a, b, c, d, e = rand_seq(rnd, 1200), rand_seq(rnd, 50), rand_seq(rnd, 400), rand_seq(rnd, 700), rand_seq(rnd, 600)
    chain = ("chain 1 a 1200 + 100 1200 a 1200 + 100 1200 1\n500 0 0\n600\n\n"           # idx 0 and the last idx of the first block; the second ends on the contig's last base
             "chain 2 b 50 + 10 12 b 50 + 10 12 2\n2\n\n"                                # a 2-base chain
             "chain 3 c 400 + 0 150 c 400 + 0 150 3\n60 10 10\n80\n\n"                     # both blocks small and the last one broken at its last base: the header alone
             "chain 4 d 700 + 0 650 d 700 + 0 650 4\n300 20 20\n250 30 30\n50\n\n"         # a 1-field last block of 50: kept
             "chain 5 e 600 + 0 500 e 600 + 0 500 5\n500\n")                                # a mismatch at the last idx of the last block: a trailing 0
    new = [("a", sub(a, [100, 599, 900])), ("b", sub(b, [11])), ("c", sub(c, [149])), ("d", sub(d, [330])), ("e", sub(e, [499]))]
    return [("a", a), ("b", b), ("c", c), ("d", d), ("e", e)], new, chain


def fold(rnd):
    f, g = rand_seq(rnd, 4000), rand_seq(rnd, 2500)
    at = [50, 150, 251, 353, 354, 355, 356, 900, 901, 1500]                              # good stretches of 50, 99, 100, 101, 0, 0, 0, 543, 0, 598 and the rest
    chain = ("chain 1 f 4000 + 0 3974 f %d + 0 3967 1\n30 5 5\n40 0 3\n2000 10 0\n99 1 1\n100 1 1\n101 1 1\n1500 2 2\n20 4 4\n60\n\n"
             "chain 2 g 2500 + 100 2400 g 2500 + 100 2400 2\n1000 100 100\n1100\n")
    # the new side of chain 1 follows its dq: built block by block
    blocks = [(30, 5, 5), (40, 0, 3), (2000, 10, 0), (99, 1, 1), (100, 1, 1), (101, 1, 1), (1500, 2, 2), (20, 4, 4), (60, 0, 0)]
    new_f, s = "", 0
    for size, dt, dq in blocks:
        new_f += f[s:s + size] + rand_seq(rnd, dq); s += size + dt
    new_f += rand_seq(rnd, 120)
    new_f = sub(new_f, [78 + k for k in at] + [78 + 2007 + 30])                          # the 2000-block starts at new 78; one mismatch in the 99-block
    return [("f", f), ("g", g)], [("f", new_f), ("g", sub(g, [100 + 999, 1200 + 1, 1200 + 2, 2299]))], chain % len(new_f)


def letters(rnd):
    s = rand_seq(rnd, 900)
    old = s[:100].lower() + s[100:200] + "NNNNnnnnRRYK*-" + s[214:600] + "acgtn" * 20 + s[700:]
    new = s[:100] + s[100:200].lower() + "nnNNNNnnRNYk*-" + s[214:600].swapcase() + "ACGTN" * 20 + s[700:]
    return [("l", old)], [("l", new)], "chain 1 l 900 + 0 880 l 900 + 0 880 1\n450 5 5\n425\n"


WORKED_BUILD = "chain\t5\tx\t2002\t+\t1\t1999\tx\t2008\t+\t1\t2004\t1\n149\t3\t3\n646\t2\t7\n394\t91\t91\n713\n"


def main():
    d = os.path.join(HERE, "g12_exact"); os.makedirs(d, exist_ok=True)
    rnd = random.Random(20261020)
    cases = [("worked", worked(rnd)), ("minus", minus(rnd)), ("minus2", minus2(rnd)), ("order", order(rnd)), ("ends", ends(rnd)), ("fold", fold(rnd)), ("letters", letters(rnd)),
             ("random", cx.random_pair())]
    stand_in = tempfile.mkdtemp(prefix="al_g12_bio_"); os.makedirs(os.path.join(stand_in, "Bio"))
    open(os.path.join(stand_in, "Bio", "__init__.py"), "w").write("")
    open(os.path.join(stand_in, "Bio", "SeqIO.py"), "w").write(SEQIO)
    meta = {}
    for name, (old, new, chain) in cases:
        files = {".old.fa": cx.fa_text(old), ".new.fa": cx.fa_text(new), ".chain": chain}
        src = tempfile.mkdtemp(prefix="al_g12_") if name == "random" else d    # (random's inputs are not committed: chainexact_cases.random_pair makes them)
        for suffix, text in files.items():
            open(os.path.join(src, name + suffix), "w").write(text)
        p = lambda suffix: os.path.join(src if suffix in files else d, name + suffix)
        m = {}
        for mode, suffix in (("verify", ".verify.txt"), ("build", ".build.chain")):
            r = subprocess.run([sys.executable, SCRIPT, mode, p(".old.fa"), p(".new.fa"), p(".chain")], env=dict(os.environ, PYTHONPATH=stand_in), capture_output=True)
            assert r.returncode == 0, r.stderr.decode()[-2000:]
            open(p(suffix), "wb").write(r.stdout)
        for suffix in (".old.fa", ".new.fa", ".chain", ".verify.txt", ".build.chain"):
            data = open(p(suffix), "rb").read()
            m[name + suffix] = hashlib.md5(data).hexdigest()
        meta[name] = m
        print("g12_exact/%s: verify %d lines, build %d lines" % (name, open(p(".verify.txt")).read().count("\n"), open(p(".build.chain")).read().count("\n")))
    assert open(os.path.join(d, "worked.build.chain")).read() == WORKED_BUILD
    assert open(os.path.join(d, "minus.verify.txt")).read() == "PASS VERIFICATION\n" and open(os.path.join(d, "minus2.verify.txt")).read().count("mismatch") == 2
    json.dump(meta, open(os.path.join(d, "meta.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()

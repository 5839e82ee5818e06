#!/usr/bin/env python3
"""Golden vectors for `tokens --gaps-bed`: a gaps BED over the fork's own test/MT-human.fa is cut into GAPS.fa by the definition of DESIGN.md 7 (what
`samtools faidx REF name:a-b` prints per row: tests/tokens_cases.py), the reference's own src/2-generate_gaps/gaps_to_fasta.py tiles it into tokens, the
reference build (oracle/_ref/mm2ref) aligns the tokens single-end.  Authoring container only (needs /root/reference); what is committed is data: the BED,
the target FASTA, the gap FASTA and the SAM.

    python tests/golden/make_g10_gaps_bed.py
"""
import gzip, hashlib, json, os, subprocess, sys, tempfile
HERE = os.path.dirname(os.path.abspath(__file__)); ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tokens_cases as tc
MM2REF = os.path.join(ROOT, "oracle", "_ref", "mm2ref")
SCRIPT = "/root/reference/src/2-generate_gaps/gaps_to_fasta.py"
MT = "/root/reference/src/minimap2-master_remapping/test/MT-human.fa"
READ_SIZE, SKIP = 100, 7
# a = 0; a plain row; a row shorter than the read; two overlapping rows; exactly R + 1 bases (a = b - R); an empty line; b clamped at the contig's end (16569)
BED = (b"MT_human\t0\t420\n" b"MT_human\t4001\t4250\tgap2\t0\t+\n" b"MT_human\t5200\t5280\n" b"MT_human\t9000\t9700\n" b"MT_human\t9500\t10300\n"
       b"MT_human\t12000\t12100\n" b"\n" b"MT_human\t7000\t7350\n" b"MT_human\t16300\t20000\n")


def gz_write(path, data):
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(data)


def main():
    tmp = tempfile.mkdtemp(prefix="al_g10_")
    lines = open(MT).read().split("\n")
    name = lines[0][1:].split()[0]; seq = "".join(l.strip() for l in lines[1:])
    gaps = tc.gaps_fasta(BED, [(name.encode(), seq)])
    # upper case in every row (the file's one lower-case base, 3107, is in none): SEQ of the BED route equals the FASTA route's
    assert name == "MT_human" and all(set(l) <= set(b"ACGTN") for l in gaps.split(b"\n") if not l.startswith(b">"))
    open(os.path.join(tmp, "gaps.fa"), "wb").write(gaps)
    # (the script ends with an IndexError on its last statement after all tokens are written: exit status ignored)
    subprocess.run([sys.executable, SCRIPT, "gaps.fa", str(READ_SIZE), "tokens.fa", str(SKIP)], cwd=tmp, check=False, stderr=subprocess.DEVNULL)
    sam = subprocess.run([MM2REF, MT, "tokens.fa"], cwd=tmp, capture_output=True, check=True).stdout
    d = os.path.join(HERE, "g10_gaps_bed"); os.makedirs(d, exist_ok=True)
    open(os.path.join(d, "gaps.bed"), "wb").write(BED)
    gz_write(os.path.join(d, "gaps.fa.gz"), gaps)
    gz_write(os.path.join(d, "MT-human.fa.gz"), open(MT, "rb").read())
    gz_write(os.path.join(d, "expected.sam.gz"), sam)
    n_tok = sum(1 for l in open(os.path.join(tmp, "tokens.fa")) if l.startswith(">"))
    rr = tc.rows(BED, [(name.encode(), len(seq))])
    assert n_tok == len(tc.tokens([n for _, _, _, n in rr], READ_SIZE, SKIP))
    json.dump({"ref": "MT-human.fa", "bed": "gaps.bed", "gaps": "gaps.fa", "read_size": READ_SIZE, "skip": SKIP, "n_tokens": n_tok, "n_sam_lines": sam.count(b"\n"),
               "sam_md5": hashlib.md5(sam).hexdigest()}, open(os.path.join(d, "meta.json"), "w"), indent=1, sort_keys=True)
    print("g10_gaps_bed:", n_tok, "tokens,", sam.count(b"\n"), "SAM lines")


if __name__ == "__main__":
    main()

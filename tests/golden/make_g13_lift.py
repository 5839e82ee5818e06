"""Writes tests/golden/g13_lift: the directed chain file of tests/lift_cases.py, two small BAMs made from its directed records, and what `lift` must make of
them according to the rules restated there -- header text, reference list, the kept records' fields and the BED rows (expected.json).

    python tests/golden/make_g13_lift.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lift_cases as lc  # noqa: E402
from select_cases import bgzf  # noqa: E402

FIELDS = ["qname", "flag", "rid", "pos", "mapq", "cigar", "nrid", "npos", "tlen", "bin", "tags"]
W = 8192


def cases():
    return {"directed257": lc.directed(257), "cut3": lc.walk_sets(W)["cut3"]}


def main():
    d = os.path.join(HERE, "g13_lift"); os.makedirs(d, exist_ok=True)
    open(os.path.join(d, "directed.chain"), "w").write(lc.CHAIN)
    tab = lc.Table(lc.CHAIN); exp = {}
    for name, recs in cases().items():
        open(os.path.join(d, name + ".bam"), "wb").write(bgzf(lc.bam_bytes(lc.HEADER, lc.REFS, recs), 0xff00))
        v, kept, rows = lc.lift_all(lc.CHAIN, lc.REFS, recs)
        exp[name] = dict(bam=name + ".bam", chain="directed.chain", header=lc.lift_header(lc.HEADER, tab), refs=[list(x) for x in zip(tab.q_names, tab.q_sizes)], fields=FIELDS,
                         records=[[lc.as_read_bam(k)[f] for f in FIELDS] for k in kept], bed="".join(x + "\n" for x in rows), verdicts=v)
    json.dump(exp, open(os.path.join(d, "expected.json"), "w"), indent=0, sort_keys=True)


if __name__ == "__main__":
    main()

"""Restatement of the fork's MD:Z / cs:Z strings and of --eqx CIGARs (format.c:137-214, align.c:169-238) in Python, for the tests of
the --MD / --cs / -Y output options: from a reference sequence, the record's POS and CIGAR, and the aligned query bases."""
import re

NT4 = {c: i for i, c in enumerate("ACGT")}
NT4.update({c.lower(): i for c, i in list(NT4.items())}); NT4["U"] = NT4["u"] = 3


def nt4(s):
    return [NT4.get(c, 4) for c in s]


def cigar_ops(cig):
    return [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cig)]


def md_cs(tseq, qseq, ops, kind="MD", long_cs=False):
    """tseq / qseq: nt4 codes of the reference window [rs, re) and of the aligned query (record's strand); ops: [(len, op)] without
    clips.  Returns the MD:Z value (kind "MD") or the cs:Z value."""
    out, q, t, l_md = [], 0, 0, 0
    for n, op in ops:
        if op in "M=X":
            run = []
            for j in range(n):
                a, b = qseq[q + j], tseq[t + j]
                if a != b:
                    if kind == "MD":
                        out.append("%d%s" % (l_md, "ACGTN"[b])); l_md = 0
                    else:
                        if run:
                            out.append("=" + "".join(run) if long_cs else ":%d" % len(run)); run = []
                        out.append("*" + "acgtn"[b] + "acgtn"[a])
                elif kind == "MD":
                    l_md += 1
                else:
                    run.append("ACGTN"[a])
            if kind != "MD" and run:
                out.append("=" + "".join(run) if long_cs else ":%d" % len(run))
            q += n; t += n
        elif op == "I":
            if kind != "MD":
                out.append("+" + "".join("acgtn"[c] for c in qseq[q:q + n]))
            q += n
        elif op == "D":
            if kind == "MD":
                out.append("%d^%s" % (l_md, "".join("ACGTN"[c] for c in tseq[t:t + n]))); l_md = 0
            else:
                out.append("-" + "".join("acgtn"[c] for c in tseq[t:t + n]))
            t += n
    if kind == "MD" and l_md > 0:
        out.append("%d" % l_md)
    return "".join(out)


def eqx(tseq, qseq, ops):
    """Each M run split into maximal = / X runs (N against N counts as =)."""
    res, q, t = [], 0, 0
    for n, op in ops:
        if op == "M":
            for j in range(n):
                o = "=" if qseq[q + j] == tseq[t + j] else "X"
                if res and res[-1][1] == o and res[-1][2]:
                    res[-1][0] += 1
                else:
                    res.append([1, o, True])
            q += n; t += n
        else:
            res.append([n, op, False])
            q += n if op == "I" else 0; t += n if op == "D" else 0
    return [(n, o) for n, o, _ in res]


def record_tag(fields, ref_seqs, kind="MD", long_cs=False):
    """The tag a SAM record (split fields) should carry, restated from its POS, CIGAR, SEQ and the reference; None if it has no
    CIGAR or no SEQ to restate from."""
    if fields[5] == "*" or fields[9] == "*" or int(fields[1]) & 4:
        return None
    ops = cigar_ops(fields[5])
    lead = ops[0][0] if ops[0][1] == "S" else 0
    core = [(n, o) for n, o in ops if o not in "SH"]
    ql = sum(n for n, o in core if o in "MI=X"); tl = sum(n for n, o in core if o in "MDN=X")
    pos = int(fields[3]) - 1
    return md_cs(nt4(ref_seqs[fields[2]][pos:pos + tl]), nt4(fields[9][lead:lead + ql]), core, kind, long_cs)


def read_fasta(path):
    seqs, name, buf = {}, None, []
    for line in open(path):
        if line.startswith(">"):
            if name is not None:
                seqs[name] = "".join(buf)
            name, buf = line[1:].split()[0], []
        else:
            buf.append(line.strip())
    if name is not None:
        seqs[name] = "".join(buf)
    return seqs


def strip_options(line):
    """A SAM record printed with --MD / --cs / --eqx / -Y, turned back into the flag-off record: tags removed, =/X runs merged into M,
    supplementary soft clips back to hard clips with SEQ/QUAL cut to the aligned part, secondary SEQ/QUAL back to '*'."""
    f = line.split("\t")
    f = f[:11] + [x for x in f[11:] if not (x.startswith("MD:Z:") or x.startswith("cs:Z:"))]
    if f[5] != "*":
        ops = []
        for n, o in cigar_ops(f[5]):
            o = "M" if o in "=X" else o
            if ops and ops[-1][1] == o == "M":
                ops[-1][0] += n
            else:
                ops.append([n, o])
        flag = int(f[1])
        if flag & 0x800 and not flag & 0x100:
            lead = ops[0][0] if ops[0][1] == "S" else 0
            trail = ops[-1][0] if ops[-1][1] == "S" else 0
            if f[9] != "*":
                f[9] = f[9][lead:len(f[9]) - trail]
                if f[10] != "*":
                    f[10] = f[10][lead:len(f[10]) - trail]
            ops = [[n, "H" if o == "S" else o] for n, o in ops]
        elif flag & 0x100:
            f[9] = f[10] = "*"
        f[5] = "".join("%d%s" % (n, o) for n, o in ops)
    return "\t".join(f)

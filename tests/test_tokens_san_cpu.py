"""The tokens of tokens --gaps-bed on the host under AddressSanitizer + UBSan: `make san-tokens` links tests/csrc/tokens_main.cpp, a stand-alone program of host
code only -- the BED row parser, the region table, the set-up kernel's twin, the runs of a batch and the SAM sink's names and bases (al_dev_tokens.h).  For
every case list of tokens_cases.py it prints the twin's table and the (start, hash) of every token in ranges of 1, 7 and all at a time, with each range's runs;
all of it is held against the plain restatement.  Nothing loaded into python is sanitized."""
import os
import subprocess

import tokens_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "airlift_amd", "csrc")


def _case_text(c):
    first, hp, toks, _ = tc.expected(c["heads"], c["src"], c["lens"], c["R"], c["S"], c["seed"])
    out = ["== %s %d %d" % (c["name"], len(c["heads"]), first[-1])] + ["T %d %d" % (first[r], hp[r]) for r in range(len(hp))]
    for chunk in (1, 7, 0):
        out.append("C %d" % chunk)
        t0 = 0
        while t0 < first[-1]:
            n = min(chunk, first[-1] - t0) if chunk else first[-1]
            out.append("G %d %d " % (t0, n) + " ".join("%d:%d" % fr for fr in tc.runs(first, t0, n)))
            out += ["%d %d" % sh for sh in toks[t0:t0 + n]]
            t0 += n
    return out


def test_token_host_code_under_asan_and_ubsan(tmp_path):
    r = subprocess.run(["make", "san-tokens"], cwd=CSRC, capture_output=True)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    cases = tc.cases(); lines = []; expect = []
    for c in cases:
        lines.append("case %s %d %d %d %d" % (c["name"], c["R"], c["S"], c["seed"], len(c["heads"])))
        lines += ["%s %d %d" % (h.decode(), s, n) for h, s, n in zip(c["heads"], c["src"], c["lens"])]
        expect += _case_text(c)
    n_bed = 0
    for c in cases:                                  # the same tables from their BED text, and the text of every token
        if "bed" not in c or c["name"] == "big":
            continue
        n_bed += 1
        lines.append("bed %s %d %d %d %d" % (c["name"], c["R"], c["S"], len(c["contigs"]), len(c["bed"])))
        lines += ["%s %d" % (n.decode(), l) for n, l in c["contigs"]] + [l.decode() for l in c["bed"]]
        expect.append("== %s" % c["name"])
        rr = tc.rows(b"\n".join(c["bed"]) + b"\n", c["contigs"]); k = 0
        for i, l in enumerate(c["bed"], 1):
            if not l.rstrip(b"\r"):
                expect.append("skip %d" % i)
            else:
                expect.append("row %d %s %d %d %d" % ((i, rr[k][0].decode()) + rr[k][1:])); k += 1
        expect += _case_text(dict(c, seed=11))
        for r_, o in tc.tokens(c["lens"], c["R"], c["S"]):
            p = c["src"][r_] + o
            expect.append("tok %s_%d %d %s" % (c["heads"][r_].decode(), o, p, "".join("ACGTN"[tc.ref_code(q)] for q in range(p, p + c["R"]))))
    for text, bad in tc.MALFORMED:                   # every malformed row is refused at its line, the rows before it are read
        n_bed += 1
        ll = text.split(b"\n")[:-1]
        lines.append("bed malformed %d %d %d %d" % (tc.R0, tc.S0, len(tc.CONTIGS), len(ll)))
        lines += ["%s %d" % (n.decode(), l) for n, l in tc.CONTIGS] + [l.decode() for l in ll]
        try:
            tc.rows(text, tc.CONTIGS); assert False, text
        except tc.BedError as e:
            assert e.line == bad
        expect.append("== malformed")
        good = tc.rows(b"\n".join(ll[:bad - 1]) + b"\n", tc.CONTIGS); k = 0
        for i, l in enumerate(ll[:bad - 1], 1):
            if not l.rstrip(b"\r"):
                expect.append("skip %d" % i)
            else:
                expect.append("row %d %s %d %d %d" % ((i, good[k][0].decode()) + good[k][1:])); k += 1
        expect += ["err %d " % bad, "refused"]
    lst = tmp_path / "list.txt"; lst.write_bytes(("\n".join(lines) + "\n").encode())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "build", "san_tokens"), str(lst)], capture_output=True, env=env)
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr).decode(errors="replace")[-3000:]
    got = r.stdout.decode().split("\n")
    assert got[-2:] == ["san_tokens: %d cases" % (len(cases) + n_bed), ""]
    assert len(got) == len(expect) + 2
    for i, e in enumerate(expect):
        assert got[i].startswith(e) if e.startswith("err ") else got[i] == e, (i, got[i][:200], e[:200])
    # what the cases are there for
    by = {c["name"]: c for c in cases}
    assert [len(range(tc.R0, n, tc.S0)) for n in by["lengths"]["lens"]] == [0, 0, 1, 1, 2]
    assert by["a0_a1"]["src"][0] == by["a0_a1"]["src"][1] and by["a0_a1"]["lens"] == [300, 300] and by["a0_a1"]["heads"] == [b"c2:0-300", b"c2:1-300"]
    assert by["b_beyond"]["lens"] == [8000 - 7799, 9000 - 8849]
    assert by["last_R1"]["src"][0] + tc.R0 + 1 == 12000 + 8000 + 9000 and tc.table(by["last_R1"]["heads"], by["last_R1"]["lens"], tc.R0, tc.S0)[0] == [0, 1, 2]
    assert tc.table(by["zero_runs"]["heads"], by["zero_runs"]["lens"], tc.R0, tc.S0)[0] == [0, 0, 0, 0, 29, 29, 29, 30, 30, 30, 30, 30]
    assert by["leading_zeros"]["heads"] == [b"c2:007-300", b"c2:7-0300"] and by["leading_zeros"]["src"] == [6, 6]
    digits = set()
    for n in ("digits_1_5_6", "digits_1_4_5_6_7", "digits_1_2_3_4"):
        digits |= {len(str(o)) for _, o in tc.tokens(by[n]["lens"], by[n]["R"], by[n]["S"])}
    assert digits == set(range(1, 8)) and len(tc.tokens(by["digits_1_5_6"]["lens"], 100, 99991)) == 11
    st = [s for s, _ in tc.expected(*[by["src_2_32"][k] for k in ("heads", "src", "lens", "R", "S", "seed")])[2]]
    assert min(st) < 2 ** 32 - 100 and any(s < 2 ** 32 < s + 100 for s in st) and any(2 ** 32 <= s < 2 ** 33 for s in st) and max(st) > 2 ** 33
    assert {s & 7 for s in by["start_and_7"]["src"]} == set(range(8)) and 50000 < tc.table(by["big"]["heads"], by["big"]["lens"], tc.R0, tc.S0)[0][-1] < 100000
    assert tc.qname_hash(b"c2:007-300_0", 100, 11) == tc.expected(*[by["leading_zeros"][k] for k in ("heads", "src", "lens", "R", "S", "seed")])[2][0][1]

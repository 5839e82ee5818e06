"""Cases and the plain restatement of `chain-exact verify|build` (run/1_build_exact_chain_file.py), shared by the CPU and the GPU tests.

A Case is what the kernels and their twin see: two texts, blocks (chain, size, dt, dq, three) in output order and chains (old0, new0, dir) -- the text offsets
of a chain's first block's first base (on a '-' chain new0 is where the new side starts and goes down from).  model() restates the function on a Case the
way the script words it: mismatches per block, the lines after pass 1, the fold of pass 2.  restate() does the same from files: the script's dict order, its
skipping rules, pass 3 and the printing.  golden() are the g12 files the script itself wrote; synthetic() are tables around the kernel's word and tile sizes."""
import json
import os
import random

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
G12 = os.path.join(HERE, "golden", "g12_exact")
_COMP = np.full(256, 255, dtype=np.uint8)
for _a, _b in ("at", "ta", "cg", "gc", "nn"):
    _COMP[ord(_a)] = ord(_b)


def _lower(a):
    return np.where((a >= 65) & (a <= 90), a | 32, a).astype(np.uint8)


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTacgtNn", "TGCAtgcaNn"))


class Case:
    def __init__(self, old=b"", new=b"", blocks=None, chains=None):
        self.old, self.new, self.blocks, self.chains = old, new, blocks or [], chains or []


def offsets(case):
    """[(old_off, new_off)] of every block"""
    out, a, b = [], 0, 0
    for i, (c, size, dt, dq, _) in enumerate(case.blocks):
        if i == 0 or case.blocks[i - 1][0] != c:
            a = b = 0
        old0, new0, d = case.chains[c]
        out.append((old0 + a, new0 - b if d else new0 + b))
        a += size + dt; b += size + dq
    return out


def lines1(case, mism):
    out = []
    for (c, size, dt, dq, three), mm in zip(case.blocks, mism):
        prev = -1
        for m in mm:
            out.append((c, m - prev - 1, 1, 1, 1)); prev = m
        out.append((c, size - prev - 1, dt, dq, three))
    return out


def pass2(l1, M):
    out, i = [], 0
    while i < len(l1):
        j = i
        while j < len(l1) and l1[j][0] == l1[i][0]:
            j += 1
        chain = l1[i:j]; c = chain[0][0]
        kept = [k for k, l in enumerate(chain) if not l[4] or l[1] >= M]
        small = lambda a, b: (sum(l[1] + l[2] for l in chain[a:b]), sum(l[1] + l[3] for l in chain[a:b]))
        if kept and kept[0] > 0:
            out.append((c, 0) + small(0, kept[0]) + (1,))
        for n, k in enumerate(kept):
            nxt = kept[n + 1] if n + 1 < len(kept) else len(chain)
            s = small(k + 1, nxt)
            out.append((c, chain[k][1], chain[k][2] + s[0], chain[k][3] + s[1], 1) if chain[k][4] else (c, chain[k][1], 0, 0, 0))
        i = j
    return out


def model(case, M=100, build=True):
    """(cnt, pos, lines1, lines2, flag); with the flag set, or without build, the lists are empty"""
    old = _lower(np.frombuffer(case.old, dtype=np.uint8)); new = _lower(np.frombuffer(case.new, dtype=np.uint8))
    mism, flag = [], 0
    for (c, size, _, _, _), (oo, no) in zip(case.blocks, offsets(case)):
        o = old[oo:oo + size]
        if case.chains[c][2]:
            n = _COMP[new[no - size + 1:no + 1][::-1]]
            flag |= int((n == 255).any())
        else:
            n = new[no:no + size]
        mism.append(np.nonzero(o != n)[0].tolist())
    if flag:
        return [0] * len(mism), [], [], [], 1
    cnt = [len(m) for m in mism]
    if not build:
        return cnt, [], [], [], 0
    pos = [(b, k) for b, mm in enumerate(mism) for k in mm]
    l1 = lines1(case, mism)
    return cnt, pos, l1, pass2(l1, M), 0


# ---- from files ------------------------------------------------------------------------------------------------------------------------------------------
def read_fa(text):
    """[(name, sequence)]: the name is the header's first word"""
    out = []
    for line in text.split("\n"):
        if line.startswith(">"):
            out.append([line[1:].split()[0], []])
        elif line and out:
            out[-1][1].append(line.strip())
    return [(n, "".join(s)) for n, s in out]


def fa_text(seqs, width=70):
    return "".join(">%s\n" % n + "".join(s[i:i + width] + "\n" for i in range(0, len(s), width)) for n, s in seqs)


def parse_chain(text):
    """[(header fields, [(size, dt, dq) | (size,)])] in the script's order: first appearance of tName, of qName inside it, of tStart inside that"""
    chains = []
    for line in text.split("\n"):
        f = line.split()
        if not f or line[0] == "#":
            continue
        if f[0] == "chain":
            chains.append((f, []))
        else:
            chains[-1][1].append(tuple(int(x) for x in f))
    t_rank, q_rank = {}, {}
    for f, _ in chains:
        t_rank.setdefault(f[2], len(t_rank)); q_rank.setdefault((f[2], f[7]), len(q_rank))
    return sorted(chains, key=lambda c: (t_rank[c[0][2]], q_rank[(c[0][2], c[0][7])]))


def table(old, new, chain_text, mode):
    """(Case, the headers of its chains) of two FASTA texts and a chain file, as the script walks them in `mode`"""
    fo, fn = read_fa(old), read_fa(new)
    off = lambda fa: {n: (sum(len(s) for _, s in fa[:i]), len(s)) for i, (n, s) in enumerate(fa)}
    oo, no = off(fo), off(fn)
    case = Case("".join(s for _, s in fo).encode(), "".join(s for _, s in fn).encode()); hdrs = []
    for f, lines in parse_chain(chain_text):
        hdrs.append(f)
        c = len(hdrs) - 1; case.chains.append((0, 0, 0))
        if f[2] not in oo or f[7] not in no:
            assert mode == "verify"
            continue
        minus = f[9] == "-"
        sfrom = int(f[5]); tfrom = int(f[8]) - int(f[10]) - 1 if minus else int(f[10])
        case.chains[c] = (oo[f[2]][0] + sfrom, no[f[7]][0] + tfrom, 1 if minus else 0)
        for l in lines:
            size, dt, dq = l[0], (l[1] if len(l) == 3 else 0), (l[2] if len(l) == 3 else 0)
            if mode == "verify" and (oo[f[2]][1] < sfrom + size + 1 or (not minus and no[f[7]][1] < tfrom + size + 1)):
                break
            case.blocks.append((c, size, dt, dq, 1 if len(l) == 3 else 0))
            sfrom += size + dt; tfrom += -(size + dq) if minus else size + dq
    return case, hdrs


def restate(mode, old, new, chain_text, M=100):
    """the bytes the script prints"""
    case, hdrs = table(old, new, chain_text, mode)
    cnt, _, _, l2, flag = model(case, M, mode == "build")
    assert not flag
    if mode == "verify":
        out = ["mismatch: %d errors in %d blocktarget: %s header: %s\n" % (k, b[1], hdrs[b[0]][7], " ".join(hdrs[b[0]])) for k, b in zip(cnt, case.blocks) if k]
        return "".join(out or ["PASS VERIFICATION\n"]).encode()
    out = []
    for c, f in enumerate(hdrs):
        f = list(f); lines = [l for l in l2 if l[0] == c]
        if lines and lines[0][4] and lines[0][1] == 0:
            f[5] = str(int(f[5]) + lines[0][2]); f[10] = str(int(f[10]) + lines[0][3]); f[11] = str(int(f[11]))
            lines = lines[1:]
        if lines and not lines[-1][4] and lines[-1][1] == 0:
            lines = lines[:-1]
            if lines:
                z = lines[-1]
                f[6] = str(int(f[6]) - z[2]); f[10] = str(int(f[10])); f[11] = str(int(f[11]) - z[3])
                lines[-1] = (c, z[1], 0, 0, 0)
        out.append(("\n" if c else "") + "\t".join(f) + "\n")
        out += ["%d\t%d\t%d\n" % l[1:4] if l[4] else "%d\n" % l[1] for l in lines]
    return "".join(out).encode()


def random_pair(seed=20261020):
    """The inputs of the golden case `random`: (old contigs, new contigs, chain text) -- five contigs of 100 000 to 300 000 bases, about 300 blocks, substitutions
    at 0.1 %.  A megabyte and a half of FASTA, so it is not committed: it is made here from numpy's frozen RandomState stream, the script's outputs for it are
    committed, and meta.json holds the md5 of the three files as the script read them."""
    rs = np.random.RandomState(seed); ri = lambda a, b: int(rs.randint(a, b))
    letters = lambda alphabet, n: np.frombuffer(alphabet, dtype=np.uint8)[rs.randint(0, len(alphabet), n)]
    other = np.full(256, ord("A"), dtype=np.uint8)
    for a, b in ("AC", "CG", "GT", "TA", "aC", "cG", "gT", "tA"):
        other[ord(a)] = ord(b)
    old, new, out = [], [], []
    for i in range(5):
        L = ri(100000, 300001); s = letters(b"ACGTacgtN" if i == 4 else b"ACGT", L)
        pos = start = ri(0, 300); t = [letters(b"ACGT", ri(0, 200))]; qpos = q0 = len(t[0]); lines = []
        while pos + 13000 < L:
            size = (ri(1, 150), ri(100, 3000), ri(2000, 9000))[ri(0, 3)]
            dt, dq = ((0, ri(1, 40)), (ri(1, 40), 0), (ri(0, 300), ri(0, 300)))[ri(0, 3)]
            t += [s[pos:pos + size], letters(b"ACGT", dq)]; lines.append("%d %d %d" % (size, dt, dq)); pos += size + dt; qpos += size + dq
        size = ri(50, 3000); t += [s[pos:pos + size], letters(b"ACGT", ri(1, 500))]; lines.append("%d" % size); pos += size; qpos += size
        q = np.concatenate(t); at = rs.randint(0, len(q), len(q) // 1000); q[at] = other[q[at]]
        old.append(("r%d" % i, s.tobytes().decode())); new.append(("q%d" % i, q.tobytes().decode()))
        out.append("chain %d r%d %d + %d %d q%d %d + %d %d %d\n" % (ri(1, 10 ** 6), i, L, start, pos, i, len(q), q0, qpos, i + 1) + "\n".join(lines) + "\n")
    return old, new, "\n".join(out)


_made = {}


def golden_path(fn):
    """a file of tests/golden/g12_exact; the three inputs of `random` are made on first use, in a directory that lives as long as the process"""
    p = os.path.join(G12, fn)
    if os.path.exists(p) or not fn.startswith("random."):
        return p
    if not _made:
        import atexit, shutil, tempfile
        d = tempfile.mkdtemp(prefix="al_g12_random_"); atexit.register(shutil.rmtree, d, True)
        old, new, chain = random_pair()
        for suffix, text in ((".old.fa", fa_text(old)), (".new.fa", fa_text(new)), (".chain", chain)):
            open(os.path.join(d, "random" + suffix), "w").write(text)
        _made["dir"] = d
    return os.path.join(_made["dir"], fn)


def golden():
    """[(name, {old, new, chain: paths}, {verify, build: expected bytes})] of tests/golden/g12_exact"""
    meta = json.load(open(os.path.join(G12, "meta.json")))
    out = []
    for name in sorted(meta):
        p = lambda suffix: golden_path(name + suffix)
        out.append((name, dict(old=p(".old.fa"), new=p(".new.fa"), chain=p(".chain")), dict(verify=open(p(".verify.txt"), "rb").read(), build=open(p(".build.chain"), "rb").read())))
    return out


# ---- synthetic tables ------------------------------------------------------------------------------------------------------------------------------------
class Builder:
    """Chains laid one behind the other into two texts; every chain's stretch starts on a 16-byte boundary of both texts plus the residues asked for."""

    def __init__(self, seed, alphabet="ACGTacgtNn"):
        self.rnd = random.Random(seed); self.old, self.new = [], []; self.n_old = self.n_new = 0; self.case = Case(); self.alphabet = alphabet

    def _bases(self, n):
        return "".join(self.rnd.choice(self.alphabet) for _ in range(n))

    def _put(self, which, s):
        if which == 0:
            self.old.append(s); self.n_old += len(s)
        else:
            self.new.append(s); self.n_new += len(s)

    def chain(self, blocks, minus=False, r_old=0, r_new=0, align=True):
        """blocks: [(size, dt, dq, mismatch indices)], dt None on the 1-field line; r_old / r_new: residues mod 16 of the first block's first base (its last base,
        on the new side of a '-' chain)"""
        if align:
            self._put(0, self._bases(-self.n_old % 16 + r_old)); self._put(1, self._bases(-self.n_new % 16))
        c = len(self.case.chains); image = []
        old0 = self.n_old
        for size, dt, dq, mism in blocks:
            s = self._bases(size); t = list(s.swapcase() if self.rnd.randrange(2) else s)
            for k in mism:
                t[k] = self.rnd.choice([x for x in "ACGT" if x != s[k].upper()])
                if s[k] in "Nn":
                    t[k] = "A"
            self._put(0, s + self._bases(dt or 0)); image.append("".join(t) + self._bases(dq or 0))
            self.case.blocks.append((c, size, dt or 0, dq or 0, 0 if dt is None else 1))
        image = "".join(image)
        if minus:
            lead = (r_new - (len(image) - 1)) % 16
            self._put(1, self._bases(lead)); new0 = self.n_new + len(image) - 1; self._put(1, revcomp(image))
        else:
            self._put(1, self._bases(r_new)); new0 = self.n_new; self._put(1, image)
        self.case.chains.append((old0, new0, 1 if minus else 0))

    def done(self, tail=0):
        self._put(0, self._bases(tail)); self._put(1, self._bases(tail))
        self.case.old = "".join(self.old).encode(); self.case.new = "".join(self.new).encode()
        return self.case


def edge_idx(size, tile, r_old):
    """the places of a block where the kernel can go wrong: its first and last base, both sides of every tile edge and of the first 16-byte word edges"""
    want = {0, size - 1, 15, 16, (16 - r_old) % 16, (15 - r_old) % 16, 16 + (16 - r_old) % 16}
    for k in range(tile, size + 1, tile):
        want |= {k - 1, k}
    return sorted(x for x in want if 0 <= x < size)


def sizes(tile):
    return [1, 15, 16, 17, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1]


def synthetic(tile):
    """[(name, Case, M)]"""
    out = []
    for minus in (False, True):
        tag = "minus" if minus else "plus"
        for what in ("edges", "every", "none"):
            b = Builder(len(tag) * 31 + len(what))
            for k, size in enumerate(sizes(tile)):
                r_old, r_new = (3 * k + 1) % 16, (7 * k + 5) % 16
                mism = edge_idx(size, tile, r_old) if what == "edges" else list(range(size)) if what == "every" else []
                b.chain([(size, 2, 3, mism), (size, None, None, mism[:1])], minus, r_old, r_new)
            out.append(("%s_sizes_%s" % (tag, what), b.done(tail=5), 100))
        b = Builder(7 + minus)
        for ro in range(16):
            for rn in range(16):
                b.chain([(37, None, None, [0, 15 - ro if ro < 15 else 1, 16, 36])], minus, ro, rn)
        out.append(("%s_residues" % tag, b.done(), 100))
        # a block at text offset 0 and one that ends on the texts' last byte
        b = Builder(11 + minus)
        b.chain([(tile + 5, 0, 0, [0, tile + 4]), (33, None, None, [32])], minus, 0, 0, align=False)
        b.chain([(200, 1, 0, [0]), (tile + 19, None, None, [0, tile + 18])], minus, 9, 4)
        out.append(("%s_text_ends" % tag, b.done(tail=0), 100))
    # pass 2: good stretches of 99, 100 and 101 bases, runs of adjacent mismatches, small lines leading and trailing, chains of one line, kept lines adjacent
    b = Builder(21)
    b.chain([(50, 5, 7, []), (60, 0, 9, [3]), (1000, 4, 4, [99, 200, 300, 401, 402, 403, 404, 900, 999]), (120, 3, 0, []), (130, 2, 2, []), (40, 1, 1, [39]), (70, None, None, [])])
    b.chain([(300, None, None, [])])
    b.chain([(1, None, None, [0])])
    b.chain([(2, None, None, [0, 1])])
    b.chain([(250, 10, 20, [100, 201]), (99, 1, 1, []), (100, 2, 2, []), (101, 3, 3, []), (500, None, None, [499])], minus=True, r_old=5, r_new=11)
    b.chain([(150, 0, 5, []), (150, 5, 0, []), (10, None, None, [])])
    fold = b.done(tail=3)
    for M in (1, 100, 5000):
        out.append(("fold_M%d" % M, fold, M))
    rnd = random.Random(5); b = Builder(31)
    for _ in range(40):
        blocks = []
        for j in range(rnd.randrange(1, 9)):
            size = rnd.choice([rnd.randrange(1, 40), rnd.randrange(1, 600), rnd.randrange(tile - 20, tile + 20), rnd.randrange(1, 3 * tile)])
            mism = sorted(set(rnd.randrange(size) for _ in range(rnd.choice([0, 0, 1, 3, size // 50 + 1]))))
            blocks.append((size, rnd.randrange(0, 30), rnd.randrange(0, 30), mism))
        s, _, _, m = blocks[-1]; blocks[-1] = (s, None, None, m)
        b.chain(blocks, rnd.randrange(3) == 0, rnd.randrange(16), rnd.randrange(16), align=rnd.randrange(2) == 0)
    out.append(("random", b.done(tail=rnd.randrange(16)), 100))
    return out


def minus_with_an_R(tile):
    b = Builder(41, alphabet="ACGT")
    b.chain([(tile + 3, 2, 2, [5]), (90, None, None, [])], True, 3, 6)
    c = b.done(tail=4)
    new = bytearray(c.new); new[c.chains[0][1] - tile - 1] = ord("R"); c.new = bytes(new)
    return c


# ---- the test taps (al_dbg_chainexact / al_dbg_chainexact_host) ---------------------------------------------------------------------------------------------
def tap(fn, case, M=100, build=True):
    """(cnt, pos, lines1, lines2, flag) of a Case through a tap"""
    import ctypes as C
    u32 = lambda v: np.ascontiguousarray(np.array(v, dtype=np.uint32)); u64 = lambda v: np.ascontiguousarray(np.array(v, dtype=np.uint64))
    p32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32)); p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    old = np.frombuffer(case.old, dtype=np.uint8).copy(); new = np.frombuffer(case.new, dtype=np.uint8).copy()
    p8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    n = len(case.blocks); cols = [u32([b[k] for b in case.blocks]) for k in range(5)]
    ch = [u64([c[0] for c in case.chains]), u64([c[1] for c in case.chains]), u32([c[2] for c in case.chains])]
    total = sum(b[1] for b in case.blocks)
    cap_pos = total + 1; cap_l = total + n + 1
    o_cnt = np.zeros(n + 1, dtype=np.uint32); o_pos = np.zeros(2 * cap_pos, dtype=np.uint32); o_l1 = np.zeros(5 * cap_l, dtype=np.uint32); o_l2 = np.zeros(5 * cap_l, dtype=np.uint32)
    n_pos, n_l1, n_l2, flag = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    rc = fn(p8(old), len(old), p8(new), len(new), n, p32(cols[0]), p32(cols[1]), p32(cols[2]), p32(cols[3]), p32(cols[4]), len(case.chains), p64(ch[0]), p64(ch[1]), p32(ch[2]),
            1 if build else 0, M, p32(o_cnt), p32(o_pos), cap_pos, C.byref(n_pos), p32(o_l1), cap_l, C.byref(n_l1), p32(o_l2), cap_l, C.byref(n_l2), C.byref(flag))
    assert rc == 0, rc
    rows = lambda a, k, w: [tuple(x) for x in a[:w * k].reshape(-1, w).tolist()]
    return o_cnt[:n].tolist(), rows(o_pos, n_pos.value, 2), rows(o_l1, n_l1.value, 5), rows(o_l2, n_l2.value, 5), flag.value

"""Cases and the plain restatement of the chain file's region logic (`chain-beds`, `tokens --chain`), shared by the CPU and the GPU tests.

A Table is a parsed chain file: per alignment line chain / size / dt / three, per chain c_slot / c_tstart, per slot (the distinct tNames in order of
their first header) names / L.  gaps(), constant() and retired() restate what 2_get_updated_regions_bed.py, get_constant_regions.py and
get_retired_regions.py compute, the way the scripts do it: dictionaries in insertion order, a stable sort by start, one loop that compares with the
current region's end.  cases() are the g11 golden files parsed and synthetic tables around the kernels' block and tile sizes."""
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
G11 = os.path.join(HERE, "golden", "g11_chain")
SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097)
BIG = 70000


class Table:
    def __init__(self):
        self.chain, self.size, self.dt, self.three = [], [], [], []
        self.c_slot, self.c_tstart = [], []
        self.names, self.L = [], []

    def header(self, name, tsize, tstart):
        if name not in self.names:
            self.names.append(name); self.L.append(tsize)
        self.c_slot.append(self.names.index(name)); self.c_tstart.append(tstart)

    def line(self, size, dt=None):
        self.chain.append(len(self.c_slot) - 1); self.size.append(size); self.dt.append(dt or 0); self.three.append(0 if dt is None else 1)

    def n(self):
        return len(self.chain)


def parse(text):
    """a well-formed chain file -> Table"""
    t = Table()
    for line in text.split("\n"):
        f = line.split()
        if not f or line[0] == "#":
            continue
        if f[0] == "chain":
            t.header(f[2], int(f[3]), int(f[5]))
        else:
            t.line(int(f[0]), int(f[1]) if len(f) == 3 else None)
    return t


def parse_merged(text):
    return [(f[0], int(f[1]), int(f[2])) for f in (l.split() for l in text.split("\n")) if f]


def starts(t):
    T, prev, pos = [], None, 0
    for i, c in enumerate(t.chain):
        if c != prev:
            pos, prev = t.c_tstart[c], c
        T.append(pos); pos += t.size[i] + t.dt[i]
    return T


def pad(a, b, p, L):
    return [a - p if a >= p else 0, b + p if b + p <= L - 1 else L - 1]


def interval_merge(v, strict):
    out = []
    for s, e in sorted(v, key=lambda x: x[0]):
        if out and (s < out[-1][1] if strict else s <= out[-1][1]):
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return out


def gaps(t, R, E):
    """[(slot, start, end)]"""
    T = starts(t); per = {}
    for i in range(t.n()):
        s = t.c_slot[t.chain[i]]
        per.setdefault(s, [])
        if t.three[i]:
            g = T[i] + t.size[i]
            per[s].append(pad(g, g + t.dt[i] - 1, R + E, t.L[s]))
    return [(s, a, b) for s in sorted(per) for a, b in interval_merge(per[s], True)]


def constant(t):
    T = starts(t)
    return sorted(((t.c_slot[t.chain[i]], T[i], T[i] + t.size[i] - 1) for i in range(t.n())), key=lambda x: x[0])


def retired_slots(t, M):
    """the names of the retired step's slots: M's contigs in order of first appearance, then the chain's other tNames"""
    order = []
    for name, _, _ in M:
        if name not in order:
            order.append(name)
    return order + [n for n in t.names if n not in order]


def retired(t, M, R):
    """[(slot of the retired step, start, end)]"""
    order = retired_slots(t, M); L = {n: l for n, l in zip(t.names, t.L)}; T = starts(t)
    per = {n: [] for n in order}
    for name, s, e in M:
        per[name].append(pad(s, e, R, L[name]))
    for i in range(t.n()):
        name = t.names[t.c_slot[t.chain[i]]]
        per[name].append(pad(T[i], T[i] + t.size[i] - 1, R, L[name]))
    rows = []
    for k, name in enumerate(order):
        reg = interval_merge(per[name], False); holes = []
        for j, (s, e) in enumerate(reg):
            if j == 0:
                if s > 0:
                    holes.append((0, s - 1))
            elif s - 1 >= reg[j - 1][1] + 1:
                holes.append((reg[j - 1][1] + 1, s - 1))
        if holes and reg[-1][1] < L[name] - 1:
            holes.append((reg[-1][1] + 1, L[name] - 1))
        rows += [(k, a, b) for a, b in holes]
    return rows


def bed(rows, names):
    return "".join("%s\t%d\t%d\n" % (names[s], a, b) for s, a, b in rows).encode()


def chain_text(t):
    """the Table as a chain file (every chain's header, its lines, a blank line)"""
    out, prev = [], None
    for i in range(t.n()):
        c = t.chain[i]
        if c != prev:
            if prev is not None:
                out.append("")
            s = t.c_slot[c]; prev = c
            out.append("chain 1 %s %d + %d 0 q%s %d + 0 0 %d" % (t.names[s], t.L[s], t.c_tstart[c], t.names[s], t.L[s], c + 1))
        out.append("%d %d 0" % (t.size[i], t.dt[i]) if t.three[i] else "%d" % t.size[i])
    return "\n".join(out) + "\n"


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
def golden():
    """[(name, chain text, merged text, R, E, {kind: expected bytes})] of tests/golden/g11_chain"""
    meta = json.load(open(os.path.join(G11, "meta.json")))
    out = []
    for name in sorted(meta):
        rd = lambda suffix, mode="r": open(os.path.join(G11, name + suffix), mode).read()
        out.append((name, rd(".chain"), rd(".merged.bed"), meta[name]["read_size"], meta[name]["max_errors"],
                    {k: rd(".%s.bed" % k, "rb") for k in ("gaps", "constant", "retired")}))
    return out


def _one_chain(n, size, dt):
    t = Table(); t.header("s0", n * (size + dt) + 500, 100)
    for i in range(n):
        t.line(size, dt if i + 1 < n else None)
    return t


def _chain_per_line(n):
    """every line a chain of its own (a 3-field line that no 1-field line follows), the tNames interleaved"""
    t = Table()
    for i in range(n):
        t.header("s%d" % (i % 3), 50 * n + 1000, 50 * i + (i % 7)); t.line(20, 5)
    return t


def _boundaries():
    """4 200 lines; a new chain starts at every line index of SIZES, every third on another contig"""
    t = Table(); pos = [0, 0, 0]
    for i in range(4200):
        if i == 0 or i in SIZES:
            k = sum(1 for b in SIZES if b <= i) % 3
            t.header("b%d" % k, 200000, pos[k])
        t.line(9, 3 + (i % 5)); pos[k] += 9 + 3 + (i % 5)
    return t


def _equal_starts(long_first):
    """two gaps whose padded starts are both clamped to 0, with different ends, in both input orders; the same at the contig's end for the blocks"""
    t = Table(); t.header("q", 400, 0)
    for dt in ((50, 2) if long_first else (2, 50)):
        t.line(3, dt)
    t.line(10)
    t.header("q", 400, 300)                                               # blocks [300, 349] and [352, 399]: both padded ends clamp to 399
    t.line(50, 2); t.line(48)
    return t


def _single_points():
    """R + E = 1: two chains that end with an insertion at the contig's last base give the same one-base row twice -- the strict rule does not join them"""
    t = Table()
    t.header("p", 100, 10); t.line(40, 1); t.line(49, 0)                  # gap [50, 50] -> [49, 51]; the empty gap at 100 -> [99, 99]
    t.header("p", 100, 90); t.line(10, 0)                                 # the empty gap at 100 again
    t.header("p", 100, 60); t.line(38, 1)                                 # gap [98, 98] -> [97, 99]: joins the first [99, 99]?  no: sorted before both, 99 < 99 is false
    return t


def _random(seed, n):
    rnd = random.Random(seed); t = Table(); Ls = [rnd.randrange(8 * n, 12 * n) * 40 for _ in range(4)]; at = [0] * 4
    while t.n() < n:
        c = rnd.randrange(4)
        if Ls[c] - at[c] < 4000:
            continue
        pos = at[c] + rnd.randrange(0, 300); t.header("r%d" % c, Ls[c], pos)
        for j in range(min(rnd.randrange(1, 200), n - t.n())):
            size = rnd.randrange(1, 400); dt = rnd.choice([0, 0, 1, rnd.randrange(0, 250)])
            if pos + size + dt + 3000 > Ls[c] or rnd.randrange(40) == 0:
                t.line(size); pos += size
                break
            t.line(size, dt); pos += size + dt
        at[c] = max(at[c], pos - rnd.choice([0, 0, 0, 100]))              # (now and then the next chain overlaps this one)
    M = []
    for _ in range(n // 20 + 3):
        c = [2, 0, 1][rnd.randrange(3)]; s = rnd.randrange(0, Ls[c]); M.append(("r%d" % c, s, s + rnd.randrange(0, 2000)))
    return t, M


_cases = None


def cases():
    """[(name, Table, R, E, M)]; M: merged rows (contig, start, end) of the retired step, [] for none"""
    global _cases
    if _cases is not None:
        return _cases
    c = []
    for name, chain, merged, R, E, _ in golden():
        c.append(("g11_" + name, parse(chain), R, E, parse_merged(merged)))
    for n in SIZES + (BIG,):
        c.append(("all_merge_%d" % n, _one_chain(n, 5, 3), 10, 2, [("s0", 7, 9)]))
        c.append(("none_merge_%d" % n, _one_chain(n, 100, 30), 10, 0, []))
    for n in SIZES:
        c.append(("chain_per_line_%d" % n, _chain_per_line(n), 4, 1, [("s%d" % ((n - 1) % 3), 0, 3), ("s0", 5, 5)]))
    c.append(("boundaries", _boundaries(), 2, 1, [("b1", 100000, 100010)]))
    c.append(("equal_starts_short_first", _equal_starts(False), 90, 10, [("q", 0, 5), ("q", 0, 2)]))
    c.append(("equal_starts_long_first", _equal_starts(True), 90, 10, [("q", 0, 2), ("q", 0, 5)]))
    c.append(("single_points", _single_points(), 1, 0, []))
    t, M = _random(5, BIG); c.append(("random_%d" % BIG, t, 120, 7, M))
    t, M = _random(6, 3000); c.append(("random_3000", t, 1, 0, M))
    _cases = c
    return c


# ---- malformed chain files: (text, the line that is refused) -------------------------------------------------------------------------------------------
HDR = "chain 1 cA 5000 + 100 600 qA 5000 + 0 500 1\n"
MALFORMED = [("100 5 5\n" + HDR + "100\n", 1),                            # a data line before the first header
             (HDR + "100 5\n", 2), (HDR + "100 5 5 5\n", 2),              # a field count other than 1 or 3
             (HDR + "100 x 5\n", 2), (HDR + "-100 5 5\n", 2), (HDR + "100 5 5.0\n", 2), (HDR.replace("5000 + 100", "50k + 100") + "100\n", 1),   # a non-numeric field
             (HDR + "# c\n\n0 5 5\n", 4), (HDR + "0\n", 2),               # size == 0
             (HDR + "100\n\n# c\n200\n", 5), (HDR + "100\n50 1 1\n", 3),  # a line after the chain's 1-field line
             (HDR.replace("cA 5000", "cA 2147483648") + "100\n", 1),     # tSize >= 2^31
             (HDR.replace("5000 + 100", "5000 - 100") + "100\n", 1),     # tStrand
             (HDR + "4000 10 0\n1000\n", 3), (HDR + "4000 901 0\n", 2), (HDR + "100\n" + HDR.replace("+ 100", "+ 5000") + "1\n", 4),   # a block or gap beyond tSize
             ("chain 1 cA 5000 + 100\n100\n", 1)]                         # a header cut short
MERGED_MALFORMED = [("cA\t10\n", 1), ("cA\t10\tx\n", 1), ("cA\t10\t20\ncX\t1\t2\n", 2), ("cA\t30\t20\n", 1), ("\ncA\t5000\t5001\n", 2)]


# ---- the test taps (al_dbg_chainreg / al_dbg_chainreg_host) ---------------------------------------------------------------------------------------------
def tap(fn, t, R, E, M=None):
    """(gaps, constant, retired) of Table t through a tap, as lists of (slot, start, end); retired is None without M (M = []: the blocks alone)"""
    import ctypes as C
    import numpy as np
    u32 = lambda v: np.ascontiguousarray(np.array(v, dtype=np.uint32))
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    n = t.n(); cols = [u32(x) for x in (t.chain, t.size, t.dt, t.three, t.c_slot, t.c_tstart, t.L)]
    og, oc = np.zeros(3 * n + 3, dtype=np.uint32), np.zeros(3 * n + 3, dtype=np.uint32)
    ng, nc, nr = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    if M is None:
        m_cols = [u32([])] * 3; n_m = 0; order = []; rslot_of = u32([]); RL = u32([]); o_r = u32([]); nr_p = None
    else:
        order = retired_slots(t, M); L = dict(zip(t.names, t.L)); n_m = len(M)
        m_cols = [u32([order.index(c) for c, _, _ in M]), u32([s for _, s, _ in M]), u32([e for _, _, e in M])]
        rslot_of = u32([order.index(c) for c in t.names]); RL = u32([L[c] for c in order])
        o_r = np.zeros(6 * (n + n_m) + 6, dtype=np.uint32); nr_p = C.byref(nr)
    rc = fn(n, p(cols[0]), p(cols[1]), p(cols[2]), p(cols[3]), len(t.c_slot), p(cols[4]), p(cols[5]), len(t.L), p(cols[6]),
            n_m, p(m_cols[0]), p(m_cols[1]), p(m_cols[2]), len(order), p(rslot_of), p(RL), R, E, p(og), C.byref(ng), p(oc), C.byref(nc), p(o_r), nr_p)
    assert rc == 0, rc
    rows = lambda a, k: [tuple(x) for x in a[:3 * k].reshape(-1, 3).tolist()]
    return rows(og, ng.value), rows(oc, nc.value), None if M is None else rows(o_r, nr.value)

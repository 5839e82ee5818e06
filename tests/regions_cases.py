"""Cases and the plain restatement of the region merge of `tokens --regions-bed / --merged-bed`, shared by the CPU and the GPU tests.

An interval is (group, contig index, start, end); a case names its contigs, and their rank is the place of the NAME in byte order.  merge() is the
restatement: sort the tuples, one loop.  sam_intervals() reads the intervals off a SAM text the way `samtools view -F4 | convert2bed` would."""
import random
import re

NAMES = [b"c2", b"cA", b"c10"]          # byte order: c10, c2, cA -- not the index order
SIZES = (63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
TOP = 2 ** 31 - 2


def ranks(names):
    order = sorted(set(names))
    return [order.index(n) for n in names], order


def merge(ivs, names, per_gap=True):
    """[(group, rank, start, end)] of the merged regions, in output order."""
    rk, _ = ranks(names)
    out = []
    for g, r, s, e in sorted((g if per_gap else 0, rk[c], s, e) for g, c, s, e in ivs):
        if out and out[-1][0] == g and out[-1][1] == r and s <= out[-1][3]:
            out[-1][3] = max(out[-1][3], e)
        else:
            out.append([g, r, s, e])
    return [tuple(x) for x in out]


def bed(regions, names):
    _, order = ranks(names)
    return b"".join(b"%s\t%d\t%d\n" % (order[r], s, e) for _, r, s, e in regions)


def _long_nested():
    v = [(0, 0, 1000, 100000)]
    rnd = random.Random(7)
    for _ in range(5000):
        s = rnd.randrange(1001, 89000); v.append((0, 0, s, s + rnd.randrange(1, 300)))
    v.append((0, 0, 95000, 120000))     # inside the long one's tail, behind every short one's end: joins only if the running maximum is carried
    v.append((0, 0, 120001, 120010))    # one past the end: its own region
    return v


def _own(n):
    return [(0, 0, 10 * i, 10 * i + 9) for i in range(n)]


def _one(n):
    return [(0, 0, 10 * i, 10 * i + 15) for i in range(n)]


def _boundaries():
    """1100 overlapping intervals that would be one region; the (group, contig) segment changes at every index of SIZES of the sorted order."""
    v = []
    for i in range(1100):
        seg = sum(1 for b in SIZES if b <= i)
        v.append((seg // 3, [2, 0, 1][seg % 3], 10 * i, 10 * i + 15))      # (the contig whose name has rank seg % 3: interval i is element i of the sorted list)
    return v


def _random(seed):
    rnd = random.Random(seed); v = []
    for _ in range(70000):
        s = rnd.randrange(0, 100000)
        v.append((rnd.randrange(50), rnd.randrange(3), s, s + rnd.randrange(1, 301)))
    return v


def cases():
    """[(name, intervals, names)]; the order of a list is its append order."""
    c = [("n0", []), ("n1", [(3, 1, 5, 9)]), ("two_identical", [(0, 0, 5, 9), (0, 0, 5, 9)]),
         ("book_ended", [(0, 0, 10, 20), (0, 0, 20, 30)]), ("gap_of_one", [(0, 0, 10, 20), (0, 0, 21, 30)]),
         ("nested_first_longer", [(0, 0, 10, 100), (0, 0, 20, 30), (0, 0, 90, 95), (0, 0, 99, 101)]),
         ("long_nested", _long_nested()),
         ("two_groups_same_coords", [(1, 2, 100, 200), (0, 2, 100, 200), (1, 2, 150, 260)]),
         ("same_start_two_contigs", [(0, 0, 100, 200), (0, 1, 100, 150), (0, 2, 100, 300), (0, 1, 150, 160)]),
         ("ranks_reverse", [(0, 2, 5, 6), (0, 0, 5, 6), (0, 1, 5, 6), (1, 1, 1, 2), (1, 2, 1, 2), (1, 0, 1, 2)]),
         ("top_coordinates", [(0, 0, TOP - 10, TOP), (0, 0, TOP - 300, TOP - 10), (0, 0, 0, 1), (7, 1, TOP - 1, TOP), (7, 1, TOP - 5, TOP - 2), (2 ** 20, 2, 2 ** 30, TOP)]),
         ("boundaries", _boundaries())]
    for n in SIZES:
        c.append(("own_%d" % n, _own(n))); c.append(("one_%d" % n, _one(n)))
    c += [("random_%d" % s, _random(s)) for s in (11, 12, 13)]
    out = []
    for name, v in c:
        v = list(v)
        if name.startswith(("own_", "one_", "boundaries", "long_nested")):
            random.Random(len(v)).shuffle(v)
        out.append((name, v, NAMES))
    return out


def ref_span(cigar):
    return sum(int(n) for n, op in re.findall(rb"(\d+)([MIDNSHP=X])", cigar) if op in b"MDN=X")


def sam_intervals(sam, gap_names):
    """(group, contig index, start, end) of every mapped record of a SAM text of tokens named <gap name>_<start>, and the contig names of its @SQ lines."""
    names, v = [], []
    for line in sam.split(b"\n"):
        f = line.split(b"\t")
        if line.startswith(b"@SQ"):
            names.append(f[1][3:])
        if not line or line.startswith(b"@") or int(f[1]) & 4:
            continue
        s = int(f[3]) - 1
        v.append((gap_names.index(f[0].rsplit(b"_", 1)[0]), names.index(f[2]), s, s + ref_span(f[5])))
    return v, names

"""Directed reads for the BAM tests: cut from a reference with a fixed seed, so that the records cover what random reads rarely do."""
import random

_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def _rc(s):
    return s.translate(_COMP)[::-1]


def directed_reads(ref, seed=20240611):
    """Returns (mate 1 records, mate 2 records, single-end records), each a list of (name, seq, qual) as bytes.
    Covered: odd and even lengths; unmapped reads of one and of two bases; IUPAC codes, lowercase, U and a byte >= 128 in SEQ, on reads cut from
    both strands; chimeric reads (two distant pieces of the reference, one of them reverse-complemented in half of them) whose second piece
    becomes a hard-clipped supplementary record of odd or even length; names ending in /1 and /2; a name of exactly 254 bytes."""
    rng = random.Random(seed)
    n = len(ref)

    def cut(length):
        p = rng.randrange(1000, n - 1000 - length)
        return ref[p:p + length].upper()

    def qual(length):
        return bytes(33 + rng.randrange(1, 41) for _ in range(length))

    def spoil(s, light=False):
        """IUPAC codes, lowercase, U / u and a byte >= 128 at places far enough apart for the read still to map (light: on its own, without a mate)"""
        s = bytearray(s)
        for at, c in ((7, b"R"), (58, b"u"), (101, b"\x80")) if light else ((7, b"R"), (23, b"y"), (41, b"u"), (58, b"U"), (77, b"\x80"), (95, b"n"), (101, b"K"), (119, b"\xe9")):
            if at < len(s):
                s[at:at + 1] = c
        s[130:140] = bytes(s[130:140]).lower()
        return bytes(s)

    pe1, pe2, se = [], [], []

    def pair(name, s1, s2):
        pe1.append((name + b"/1", s1, qual(len(s1)))); pe2.append((name + b"/2", s2, qual(len(s2))))

    # plain pairs of odd and even lengths, FR, both orders of the strands
    for i, (l1, l2) in enumerate(((150, 150), (149, 150), (150, 147), (101, 76), (75, 100), (151, 33))):
        frag = cut(400)
        a, b = frag[:l1], _rc(frag[-l2:])
        pair(b"plain%d" % i, *((a, b) if i % 2 == 0 else (b, a)))
    # a mapped read whose mate is one base / two bases long (unmapped, takes the mate's position), and a pair of two such reads
    frag = cut(300); pair(b"short1", frag[:150], b"A")
    frag = cut(300); pair(b"short2", b"GT", _rc(frag[-149:]))
    pair(b"shortboth", b"C", b"TG")
    # IUPAC, lowercase, U, bytes >= 128 on both strands
    for i in range(4):
        frag = cut(420)
        a, b = spoil(frag[:150 - i]), spoil(_rc(frag[-(147 + i):]))
        pair(b"iupac%d" % i, *((a, b) if i % 2 == 0 else (b, a)))
    # chimeric reads: the second piece comes from elsewhere
    for i, (la, lb) in enumerate(((90, 61), (90, 60), (81, 70), (70, 79), (100, 51), (66, 84), (77, 72), (59, 92))):
        x, y = cut(la), cut(lb)
        if i % 2:
            y = _rc(y)
        frag = cut(350)
        chim = x + y
        pair(b"chim%d" % i, chim if i % 4 < 2 else _rc(chim), _rc(frag[-150:]))
        se.append((b"sechim%d" % i, spoil(chim, True) if i % 3 == 0 else chim, qual(len(chim))))
    # a name of exactly 254 bytes (after /1 and /2 are dropped)
    frag = cut(400)
    pair(b"N" * 254, frag[:150], _rc(frag[-150:]))
    # single-end: lengths, strands, spoiled bases, the short reads, the long name
    for i, l in enumerate((150, 149, 100, 77, 36, 35)):
        s = cut(l)
        se.append((b"se%d" % i, s if i % 2 else _rc(s), qual(l)))
    for i in range(3):
        s = spoil(cut(150 - i), i > 0)
        se.append((b"seiupac%d" % i, s if i % 2 else _rc(s), qual(len(s))))
    se.append((b"seone", b"G", qual(1))); se.append((b"setwo", b"AC", qual(2)))
    se.append((b"S" * 254, cut(150), qual(150)))
    se.append((b"seslash/1", cut(120), qual(120)))
    return pe1, pe2, se

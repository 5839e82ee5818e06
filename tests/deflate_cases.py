"""The inputs of the BGZF compressor's tests (--gpu-deflate: al_dev_deflate.h, al_deflate.hip), shared by the CPU tests of the host twin and the GPU
tests of the kernel: the smallest shapes at which the compressor can go wrong.  Everything is made from fixed seeds.  cases() returns
(name, bytes, stored) with stored = the number of stored blocks the input must give, or None where that is not pinned."""
import random
import struct

BLOCK = 0xff00
LENGTHS = [0, 1, 2, 3, 4, 5, 254, 255, 256, 257, 258, 259, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK, 3 * BLOCK + 1]
# first and last distance of every distance code (RFC 1951 3.2.5)
DIST_EDGES = sorted({1, 2, 3, 4} | {b for c in range(4, 30) for b in ((1 << (c // 2)) + (c % 2) * (1 << (c // 2 - 1)) + 1, (1 << (c // 2)) + (c % 2 + 1) * (1 << (c // 2 - 1)))})


def _rand(rng, n):
    return rng.randbytes(n)


def _letters(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choices(alphabet, k=n))


def n_blocks(n):
    return (n + BLOCK - 1) // BLOCK


def planted(fresh=False):
    """Copies of earlier random bytes over several blocks: the lengths 3..258 go round over the distances of DIST_EDGES (the first and last distance of
    every distance code), eight lengths per distance; a copy is followed by a byte that differs from what followed the original.  Which of them the parse
    takes is the function's business (a candidate is the highest earlier-chunk position of the hash, not the planted one; length 3 is below the minimum
    match): the test asks only that the buffer comes out much smaller than with fresh random bytes in place of the copies (fresh=True)."""
    rng = random.Random(77)
    out = bytearray(_rand(rng, 33000))
    lens = list(range(3, 259))
    k = 0
    for d in DIST_EDGES:
        for _ in range(8):                                   # eight lengths per distance: the 256 lengths go round over the 56 distances
            ln = lens[k % len(lens)]; k += 1
            while len(out) < d:
                out += _rand(rng, 64)
            src = len(out) - d
            copy = bytes(out[src + j % d] if src + j >= len(out) else out[src + j] for j in range(ln))
            nxt = out[src + ln] if src + ln < len(out) else copy[ln % d] if d <= ln else 0
            out += _rand(rng, ln) if fresh else copy
            out.append((nxt + 1 + rng.randrange(254)) % 256 if (nxt + 1) % 256 != nxt else 0)
            out += _rand(rng, 7)
    return bytes(out)


def all_symbols():
    """One block whose parse uses every literal and every length symbol the function can emit, 258..285 (a match is at least 4 bytes long, so symbol 257,
    length 3, never occurs).  Chunk 0 is the 256 byte values.  A 300-byte random seed follows, and from position 768 on -- two chunks behind the seed's start --
    a copy of the seed's first L bytes for L = 258 down to 4, each ended by a byte that differs from the seed's next one and a byte that names L.  A copy's
    candidate is the highest start of the seed's first four bytes in an earlier 256-byte chunk: the seed itself or an earlier copy, and every earlier copy is
    longer, so the match is exactly L bytes long; the two bytes before a copy occur nowhere else, so no match starts in front of it and swallows its start."""
    rng = random.Random(286)
    seed = rng.randbytes(300)
    out = bytearray(range(256)) + seed + bytes(768 - 556)
    for ln in range(258, 3, -1):
        out += seed[:ln] + bytes([seed[ln] ^ 0xff, ln & 255])
    assert len(out) <= BLOCK
    return bytes(out)


def cases():
    rng = random.Random(20240611)
    c = []
    for n in LENGTHS:
        c.append(("acgt_%d" % n, _letters(rng, n), None))
        c.append(("zeros_%d" % n, bytes(n), 0 if n >= 254 and (n % BLOCK == 0 or n % BLOCK >= 254) else n_blocks(n) if n <= 5 else None))   # (a last block of one byte is stored: the dynamic header alone is 168 bytes)
    for n in (1, 255, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 7):
        c.append(("random_%d" % n, _rand(rng, n), n_blocks(n) if n >= 255 else None))
    c.append(("byte_x_%d" % (BLOCK + 300), b"x" * (BLOCK + 300), 0))
    for p in (2, 3, 7, 255, 256, 257, 32768):
        unit = _rand(rng, p)
        c.append(("period_%d" % p, (unit * (2 * BLOCK // p + 2))[:BLOCK + 4321 if p < 32768 else BLOCK], 0 if p < 32768 else None))
    c.append(("acgt_2_blocks", _letters(rng, 2 * BLOCK - 11), 0))
    c.append(("two_bytes", _letters(rng, BLOCK + 999, b"\x00\xff"), 0))
    for k in (-1, 0, 1):
        pre = _rand(rng, 32768 + k)
        c.append(("window_edge_%+d" % k, pre + pre[:300], None))
    c.append(("planted", planted(), None))
    body = _rand(rng, 3000)
    c.append(("match_ends_on_last_byte", (_letters(rng, BLOCK - 3000 - 500) + body + _letters(rng, 500 - 300, b"xyz") + body[:300])[:BLOCK] + _letters(rng, 100), None))
    tail = _rand(rng, 200)
    c.append(("shared_across_boundary", _letters(rng, BLOCK - 200) + tail + tail + _letters(rng, 5000), None))
    fib, a, b = [], 1, 1
    for _ in range(40):                                       # 40 Fibonacci weights, 165 580 140 in sum: scaled to a block, the small ones stay at 1
        fib.append(a); a, b = b, a + b
    w = [max(1, f * 60000 // sum(fib)) for f in fib]
    sym = [i for i, k in enumerate(w) for _ in range(k)]
    rng.shuffle(sym)
    c.append(("fibonacci_40_literals", bytes(s + 40 for s in sym), 0))
    c.append(("all_286_symbols", all_symbols(), 0))
    c.append(("records_like", b"".join(struct.pack("<iiIIiii", 100 + i % 7, 1000 * i, 0x12345678, 150, -1, -1, 0) + b"read%06d\0" % i + _letters(rng, 75, bytes(range(0x11, 0x89, 0x11))) + bytes(rng.choices(range(2, 41), weights=[1 + (q > 30) * 20 for q in range(2, 41)], k=150)) for i in range(900)), 0))
    return c

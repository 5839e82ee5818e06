"""The inputs of the BGZF inflater's tests (--gpu-inflate: al_dev_inflate.h, al_inflate.hip), shared by the CPU tests of the host twin and the GPU tests of
the kernel.  Everything is made from fixed seeds.  A case is a BGZF byte string (a list of members, back to back) with what the inflater must make of it:

  name    the case's name
  data    the bytes
  expect  the inflated bytes of all members, concatenated (valid cases), or None
  codes   the expected status of every member the BSIZE chain reaches (0 = ok; the AL_INF_E_* numbers of al_dev_inflate.h)
  chain   0, or -2 when the chain breaks behind those members (no BC subfield, BSIZE past the end)
  raw     for a case whose defect lies in the deflate stream: that raw stream, so that the verdict can be held against Python zlib's

valid_cases() / invalid_cases() return lists of them.  The oracle of every expectation is Python's zlib (decompressobj(-15)), not the code under test."""
import collections
import functools
import random
import struct
import zlib

import deflate_cases
from deflate_cases import DIST_EDGES

BLOCK = 0xff00
E_HEADER, E_BTYPE, E_STORED, E_LENGTHS, E_SYMBOL, E_DIST, E_INPUT, E_OVER, E_SHORT, E_CRC = range(1, 11)
EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])

Case = collections.namedtuple("Case", "name data expect codes chain raw")


def member(raw, payload, before=b"", after=b"", crc=None, isize=None, bsize=None, bc=True):
    """a gzip member around the raw deflate stream `raw` of `payload`: extra subfields `before`, BC, `after`"""
    n_extra = len(before) + (6 if bc else 0) + len(after)
    total = 12 + n_extra + len(raw) + 8
    assert total <= 65536, total
    extra = before + (b"BC" + struct.pack("<HH", 2, (total - 1) if bsize is None else bsize) if bc else b"") + after
    return (b"\x1f\x8b\x08\x04" + bytes(4) + b"\x00\xff" + struct.pack("<H", len(extra)) + extra + raw +
            struct.pack("<II", zlib.crc32(payload) if crc is None else crc, len(payload) if isize is None else isize))


def subfield(tag, body):
    return tag + struct.pack("<H", len(body)) + body


def deflate_raw(payload, level=5, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(payload) + c.flush()


def zlib_verdict(raw):
    """(accepted, bytes) of a raw deflate stream by Python zlib; a stream that does not reach its end is not accepted"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(raw)
    except zlib.error:
        return False, None
    return d.eof, out


def blocks(payload):
    return [payload[o:o + BLOCK] for o in range(0, len(payload), BLOCK)]


# ---- a bit writer for hand-assembled streams (RFC 1951 3.1.1: values from the least significant bit, Huffman codes from the most significant) ----------
class Bits:
    def __init__(self):
        self.acc = 0; self.n = 0

    def bits(self, v, k):
        assert 0 <= v < (1 << k) or k == 0
        self.acc |= v << self.n; self.n += k

    def code(self, c):
        code, k = c
        for i in range(k - 1, -1, -1):
            self.bits(code >> i & 1, 1)

    def align(self):
        self.n = (self.n + 7) // 8 * 8

    def bytes(self):
        self.align()
        return self.acc.to_bytes(self.n // 8, "little")

    def stored(self, data, final=False, nlen=None):
        self.bits(1 if final else 0, 1); self.bits(0, 2); self.align()
        self.bits(len(data), 16); self.bits((len(data) ^ 0xffff) if nlen is None else nlen, 16)
        for b in data:
            self.bits(b, 8)


def canon(lens):
    """{symbol: (code, length)} of the canonical code (RFC 1951 3.2.2); no check of completeness: the cases want bad sets too"""
    code, out = 0, {}
    for ln in range(1, 16):
        for s, l in enumerate(lens):
            if l == ln:
                out[s] = (code, ln); code += 1
        code <<= 1
    return out


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in range(2)]
FIXED_L = canon([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_D = canon([5] * 32)


def len_sym(ln):
    if ln == 258:
        return 28
    return max(k for k in range(28) if LEN_BASE[k] <= ln)


def dist_sym(d):
    return max(k for k in range(30) if DIST_BASE[k] <= d)


def put_match(bw, lc, dc, ln, dist):
    k = len_sym(ln); bw.code(lc[257 + k]); bw.bits(ln - LEN_BASE[k], LEN_EXTRA[k])
    k = dist_sym(dist); bw.code(dc[k]); bw.bits(dist - DIST_BASE[k], DIST_EXTRA[k])


CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_LENS = [4] * 13 + [5] * 6               # a complete code over all 19 code-length symbols: 13/16 + 6/32 = 1


def rle(lens):
    """the code-length symbols of a sequence of lengths, greedy as zlib's: (symbol, extra value, extra bits, first index, count)"""
    out, i = [], 0
    while i < len(lens):
        j = i
        while j < len(lens) and lens[j] == lens[i]:
            j += 1
        run = j - i
        if lens[i] == 0 and run >= 3:
            k = min(run, 138)
            out.append((18, k - 11, 7, i, k) if k >= 11 else (17, k - 3, 3, i, k)); i += k
        elif lens[i] != 0 and run >= 4:
            out.append((lens[i], 0, 0, i, 1)); k = min(run - 1, 6); out.append((16, k - 3, 2, i + 1, k)); i += 1 + k
        else:
            out.append((lens[i], 0, 0, i, 1)); i += 1
    return out


def dynamic_header(bw, llens, dlens, final=True, plan=None, cl_lens=CL_LENS):
    """BFINAL, BTYPE = 2, the counts, the code-length code, and the lengths as `plan` (default: rle of llens + dlens, which runs across the boundary)"""
    cc = canon(cl_lens)
    bw.bits(1 if final else 0, 1); bw.bits(2, 2)
    bw.bits(len(llens) - 257, 5); bw.bits(len(dlens) - 1, 5); bw.bits(19 - 4, 4)
    for s in CL_ORDER:
        bw.bits(cl_lens[s], 3)
    for sym, ev, eb, _, _ in (rle(list(llens) + list(dlens)) if plan is None else plan):
        bw.code(cc[sym]); bw.bits(ev, eb)


def lit_lens(pairs, n=257):
    l = [0] * n
    for s, k in pairs:
        l[s] = k
    return l


def _hand():
    """hand-assembled members: (name, raw stream)"""
    rng = random.Random(1951)
    out = []
    # 15-bit literal codes: lengths 1, 2, ..., 14, 15, 15 (complete) over the end-of-block symbol and fifteen literals
    syms = [256] + list(range(65, 80))
    ll = lit_lens(list(zip(syms, list(range(1, 15)) + [15, 15])))
    bw = Bits(); dynamic_header(bw, ll, [1]); lc = canon(ll)
    for s in [79, 78, 65, 79, 77, 78, 66, 79] * 5:
        bw.code(lc[s])
    bw.code(lc[256]); out.append(("hand_15_bit_literals", bw.bytes()))
    # 16 across the boundary: ..., 256 and 257 have 3 bits, and so have all eight distance codes
    ll = lit_lens([(97, 1), (98, 2), (256, 3), (257, 3)], 258); dl = [3] * 8
    plan = rle(ll + dl)
    assert any(s == 16 and i < 258 < i + k for s, _, _, i, k in plan)
    bw = Bits(); dynamic_header(bw, ll, dl, plan=plan); lc, dc = canon(ll), canon(dl)
    for s in (97, 98, 97, 97):
        bw.code(lc[s])
    put_match(bw, lc, dc, 3, 1); put_match(bw, lc, dc, 3, 4); bw.code(lc[98]); bw.code(lc[256])
    out.append(("hand_repeat_16_across_boundary", bw.bytes()))
    # 17 across the boundary: 257..259 and the first three distance lengths are zero
    ll = lit_lens([(97, 1), (98, 2), (256, 2)], 260); dl = [0, 0, 0, 1, 1]
    plan = rle(ll + dl)
    assert any(s == 17 and i < 260 < i + k for s, _, _, i, k in plan)
    bw = Bits(); dynamic_header(bw, ll, dl, plan=plan); lc = canon(ll)
    for s in (97, 98, 98, 97, 256):
        bw.code(lc[s])
    out.append(("hand_repeat_17_across_boundary", bw.bytes()))
    # 18 across the boundary: 257..269 and the first four distance lengths
    ll = lit_lens([(97, 1), (98, 2), (256, 2)], 270); dl = [0, 0, 0, 0, 1, 1]
    plan = rle(ll + dl)
    assert any(s == 18 and i < 270 < i + k for s, _, _, i, k in plan)
    bw = Bits(); dynamic_header(bw, ll, dl, plan=plan); lc = canon(ll)
    for s in (98, 97, 97, 98, 256):
        bw.code(lc[s])
    out.append(("hand_repeat_18_across_boundary", bw.bytes()))
    # exactly one distance code (one bit, incomplete: zlib takes it)
    ll = lit_lens([(120, 1), (256, 2), (257 + len_sym(10), 2)], 257 + len_sym(10) + 1)
    bw = Bits(); dynamic_header(bw, ll, [1]); lc, dc = canon(ll), canon([1])
    bw.code(lc[120]); put_match(bw, lc, dc, 10, 1); bw.code(lc[120]); bw.code(lc[256])
    out.append(("hand_one_distance_code", bw.bytes()))
    # no distance code at all, literals only
    ll = lit_lens([(120, 1), (121, 2), (256, 2)])
    bw = Bits(); dynamic_header(bw, ll, [0]); lc = canon(ll)
    for s in (120, 121, 121, 120, 256):
        bw.code(lc[s])
    out.append(("hand_no_distance_code", bw.bytes()))
    # only the end-of-block symbol, one bit: an empty member (incomplete literal set of one code)
    ll = lit_lens([(256, 1)])
    bw = Bits(); dynamic_header(bw, ll, [0]); bw.code(canon(ll)[256])
    out.append(("hand_only_end_of_block", bw.bytes()))
    # length 258 at distance 1
    bw = Bits(); bw.bits(1, 1); bw.bits(1, 2); bw.code(FIXED_L[120]); put_match(bw, FIXED_L, FIXED_D, 258, 1); bw.code(FIXED_L[121]); bw.code(FIXED_L[256])
    out.append(("hand_length_258_distance_1", bw.bytes()))
    # distance 32768 from position 32768 exactly
    bw = Bits(); bw.stored(rng.randbytes(32768)); bw.bits(1, 1); bw.bits(1, 2); put_match(bw, FIXED_L, FIXED_D, 258, 32768); bw.code(FIXED_L[256])
    out.append(("hand_distance_32768_at_32768", bw.bytes()))
    # every first and last distance of a distance code, the match longer than the distance wherever a length can be
    bw = Bits(); bw.stored(rng.randbytes(33000)); bw.bits(1, 1); bw.bits(1, 2)
    for d in DIST_EDGES:
        put_match(bw, FIXED_L, FIXED_D, min(258, d + 3), d); bw.code(FIXED_L[rng.randrange(256)])
    bw.code(FIXED_L[256])
    out.append(("hand_dist_edges_overlapping", bw.bytes()))
    return out


def _one(name, raw, **kw):
    ok, payload = zlib_verdict(raw)
    assert ok, name
    return Case(name, member(raw, payload, **kw), payload, [0], 0, raw)


@functools.lru_cache(maxsize=None)
def valid_cases():
    import deflate_util
    rng = random.Random(20250613)
    c = []
    how = [("l0", 0, zlib.Z_DEFAULT_STRATEGY), ("l1", 1, zlib.Z_DEFAULT_STRATEGY), ("l5", 5, zlib.Z_DEFAULT_STRATEGY), ("l9", 9, zlib.Z_DEFAULT_STRATEGY),
           ("fixed", 5, zlib.Z_FIXED), ("huffman", 5, zlib.Z_HUFFMAN_ONLY), ("rle", 5, zlib.Z_RLE)]
    for name, payload, _ in deflate_cases.cases():
        for tag, level, strategy in how:
            bl = blocks(payload)
            if tag == "l0":
                bl = [payload[o:o + 65000] for o in range(0, len(payload), 65000)]     # (a stored member of 0xff00 bytes would not fit 65536)
            c.append(Case("%s_%s" % (name, tag), b"".join(member(deflate_raw(b, level, strategy), b) for b in bl) + EOF_BLOCK, payload, [0] * (len(bl) + 1), 0, None))
        own = deflate_util.deflate_host(payload)[0] if payload else b""
        c.append(Case("%s_own" % name, own + EOF_BLOCK, payload, [0] * (deflate_cases.n_blocks(len(payload)) + 1), 0, None))
    # several deflate blocks of different types in one member, with an empty stored block (Z_SYNC_FLUSH) and a Z_FULL_FLUSH between them
    text = deflate_cases._letters(rng, 9000); noise = rng.randbytes(3000)
    a = zlib.compressobj(9, zlib.DEFLATED, -15); b = zlib.compressobj(5, zlib.DEFLATED, -15, 9, zlib.Z_FIXED); s = zlib.compressobj(0, zlib.DEFLATED, -15)
    raw = (a.compress(text[:4000]) + a.flush(zlib.Z_SYNC_FLUSH) + a.compress(text[4000:]) + a.flush(zlib.Z_FULL_FLUSH) +
           b.compress(text[:2000]) + b.flush(zlib.Z_SYNC_FLUSH) + s.compress(noise) + s.flush())
    c.append(_one("flushes_mixed_block_types", raw))
    for n in (0, 1, 65280, 65535, 65536):
        p = deflate_cases._letters(rng, n)
        c.append(Case("payload_%d" % n, member(deflate_raw(p, 5), p), p, [0], 0, None))
    p = rng.randbytes(65536 - 18 - 5 - 8)
    bw = Bits(); bw.stored(p, final=True)
    c.append(Case("stored_member_of_65536_bytes", member(bw.bytes(), p), p, [0], 0, None))
    p = deflate_cases._letters(rng, 5000); good = member(deflate_raw(p, 5), p)
    c.append(Case("eof_block_alone", EOF_BLOCK, b"", [0], 0, None))
    c.append(Case("eof_block_in_the_middle", good + EOF_BLOCK + good + EOF_BLOCK, p + p, [0] * 4, 0, None))
    c.append(Case("eof_block_missing", good + good, p + p, [0, 0], 0, None))
    c.append(Case("extra_subfield_before_and_after", member(deflate_raw(p, 5), p, before=subfield(b"XY", b"abc"), after=subfield(b"ZZ", b"")) + EOF_BLOCK, p, [0, 0], 0, None))
    for name, raw in _hand():
        c.append(_one(name, raw))
    return c


@functools.lru_cache(maxsize=None)
def invalid_cases():
    rng = random.Random(1952)
    text = deflate_cases._letters(rng, 3000)
    c = []

    def bad(name, raw, code, payload=b"", **kw):
        c.append(Case(name, member(raw, payload, **kw), None, [code], 0, raw))

    bw = Bits(); bw.bits(1, 1); bw.bits(3, 2); bad("block_type_3", bw.bytes(), E_BTYPE)
    bw = Bits(); bw.stored(b"hello", final=True, nlen=0x1234); bad("len_nlen_mismatch", bw.bytes(), E_STORED, payload=b"hello")
    bw = Bits(); bw.stored(bytes(100), final=True); bad("stored_longer_than_input", bw.bytes()[:-90], E_INPUT, payload=bytes(100))
    bw = Bits(); dynamic_header(bw, lit_lens([(97, 1), (98, 1), (256, 1)]), [0]); bw.bits(0, 8); bad("oversubscribed_literal_set", bw.bytes(), E_LENGTHS)
    bw = Bits(); dynamic_header(bw, lit_lens([(97, 2), (256, 2)]), [0]); bw.bits(0, 8); bad("incomplete_literal_set", bw.bytes(), E_LENGTHS)
    bw = Bits(); dynamic_header(bw, lit_lens([(97, 1), (256, 1)]), [2, 2, 2]); bw.bits(0, 8); bad("incomplete_distance_set", bw.bytes(), E_LENGTHS)
    bw = Bits(); dynamic_header(bw, lit_lens([(97, 1), (256, 1)]), [0], plan=[(l, 0, 0, i, 1) for i, l in enumerate(lit_lens([(97, 1), (256, 1)]) + [0])], cl_lens=[4] * 12 + [0] * 7); bw.bits(0, 8); bad("incomplete_code_length_set", bw.bytes(), E_LENGTHS)
    ll = lit_lens([(97, 1), (256, 1)])
    bw = Bits(); dynamic_header(bw, ll, [0], plan=[(16, 0, 2, 0, 3)] + rle(ll + [0])[1:]); bw.bits(0, 8); bad("repeat_with_no_previous_length", bw.bytes(), E_LENGTHS)
    bw = Bits(); dynamic_header(bw, ll, [0], plan=rle(ll + [0])[:-1] + [(18, 127, 7, 257, 138)]); bw.bits(0, 8); bad("repeat_past_the_end", bw.bytes(), E_LENGTHS)
    bw = Bits(); dynamic_header(bw, lit_lens([(97, 1), (98, 1)]), [0]); bw.bits(0, 8); bad("missing_end_of_block_code", bw.bytes(), E_LENGTHS)
    for s in (286, 287):
        bw = Bits(); bw.bits(1, 1); bw.bits(1, 2); bw.code(FIXED_L[97]); bw.code(FIXED_L[s]); bw.bits(0, 16); bad("symbol_%d" % s, bw.bytes(), E_SYMBOL, payload=b"a")
    for s in (30, 31):
        bw = Bits(); bw.bits(1, 1); bw.bits(1, 2); bw.code(FIXED_L[97]); bw.code(FIXED_L[257]); bw.code(FIXED_D[s]); bw.bits(0, 16); bad("distance_code_%d" % s, bw.bytes(), E_SYMBOL, payload=b"aaaa")
    bw = Bits(); bw.bits(1, 1); bw.bits(1, 2); bw.code(FIXED_L[97]); put_match(bw, FIXED_L, FIXED_D, 3, 2); bw.code(FIXED_L[256]); bad("distance_beyond_the_start", bw.bytes(), E_DIST, payload=b"aaaa")
    bad("input_ends_in_mid_symbol", deflate_raw(text, 9)[:-2], E_INPUT, payload=text)
    for c_ in c:
        assert not zlib_verdict(c_.raw)[0], c_.name
    raw = deflate_raw(text, 5)
    c.append(Case("output_one_over_isize", member(raw, text, isize=len(text) - 1), None, [E_OVER], 0, None))
    c.append(Case("output_one_short_of_isize", member(raw, text, isize=len(text) + 1), None, [E_SHORT], 0, None))
    c.append(Case("wrong_crc", member(raw, text, crc=zlib.crc32(text) ^ 0x8000), None, [E_CRC], 0, None))
    good = member(raw, text)
    c.append(Case("bsize_past_the_file", good + member(raw, text, bsize=len(good) + 100), None, [0], -2, None))
    c.append(Case("no_bc_subfield", good + member(raw, text, bc=False, before=subfield(b"XY", b"ab")), None, [0], -2, None))
    return c


def is_member_level(case):
    """the defect is one bad member that the chain walks over: it can stand between two good ones"""
    return case.chain == 0 and len(case.codes) == 1 and case.codes[0] != 0

// al_dev_inflate.h -- the BGZF member inflater of --gpu-inflate as ONE function of a member's bytes, written once for both sides: the pieces below
// are compiled for the device (k_inflate, al_inflate.hip) and for the CPU (al_inflate_member_host, the twin at the end of this file, which evaluates
// the same function serially).  The twin is what the kernel is tested against byte for byte and what tests/csrc/inflate_main.cpp runs under the sanitizers.
//
// THE FUNCTION.  Input: the `msize` bytes of one gzip member (RFC 1952) whose extra field holds the BGZF subfield `BC` (SAM specification 4.1), and
// ISIZE, the last four bytes of it.  Output: ISIZE bytes and a status, 0 or one of AL_INF_E_*.  The deflate stream (RFC 1951 complete: stored, fixed and
// dynamic blocks, any number of them) lies between the header and the eight trailer bytes: csize = msize - header - 8 bytes.
//
//  1. Header.  al_inf_parse_header: magic, CM = 8, FLG = FEXTRA alone, the subfields of the extra field walked inside XLEN until `BC` (length 2) is
//     found; BSIZE + 1 is the member's size.  The same function lists the members of a file on the host (al_inf_list) without inflating anything.
//  2. Tokens.  al_inf_next turns the deflate stream into tokens, one per call: a literal byte, a match (length 3..258, distance 1..32768) or the run of a
//     stored block.  Every token is checked BEFORE it is handed out: a match's distance does not reach in front of the member's first byte, and the
//     output position after the token is at most ISIZE.  The caller writes a token's bytes without any further test.
//  3. Code lengths.  al_inf_check_lengths judges a set of code lengths as zlib's inflate_table does: an over-subscribed set is an error; an incomplete
//     set is an error unless it is a literal/length or distance set whose longest code has one bit (one code), or no code at all (a distance set of a
//     block of literals; using it is a bad symbol).  The code-length alphabet's own set must be complete.  A repeat symbol (16 / 17 / 18) may run across the
//     literal / distance boundary, not past HLIT + HDIST; 16 needs a previous length.  The end-of-block symbol must have a code.
//  4. Tables.  al_inf_build: the symbols in canonical order with the count per length (codes longer than the fast table's index are decoded from
//     these, a bit at a time), and a fast table indexed by the next AL_INF_LBITS / AL_INF_DBITS bits of the stream.  2.2 KB per decoder: LDS per wavefront.
//  5. Bounds.  The bit reader (AlInfBits) never reads a byte outside in[0, csize): past the end it delivers zero bits and counts them, and every
//     loop looks at the count (al_inf_over) once per iteration.  An iteration of any loop consumes at least one bit of input or produces at least one
//     byte of output, so 8 * csize + ISIZE bounds the iterations (+ a constant for the bits delivered past the end before the count is looked at);
//     AlInfState::iters counts them, and the sanitizer program asserts the bound.
//  6. Trailer.  The stream must end in the last byte before the trailer, the output must be ISIZE bytes, and CRC32 of them must be the trailer's.
#pragma once
#include <stdint.h>
#include <string.h>
#include "al_dev_deflate.h"       // AL_DHD, the CRC32 pieces

enum {
	AL_INF_OK = 0,
	AL_INF_E_HEADER = 1,        // not a gzip member with a BC subfield, or BSIZE does not fit the stream inside it
	AL_INF_E_BTYPE = 2,         // block type 3
	AL_INF_E_STORED = 3,        // LEN != ~NLEN
	AL_INF_E_LENGTHS = 4,       // code lengths: over-subscribed, incomplete, bad repeat, too many symbols, no end-of-block code
	AL_INF_E_SYMBOL = 5,        // a bit pattern that is no code, literal/length symbol 286 / 287, distance symbol 30 / 31
	AL_INF_E_DIST = 6,          // distance reaches in front of the member's first byte
	AL_INF_E_INPUT = 7,         // the deflate stream needs more than csize bytes
	AL_INF_E_OVER = 8,          // output over ISIZE
	AL_INF_E_SHORT = 9,         // output short of ISIZE
	AL_INF_E_CRC = 10
};
#define AL_INF_MAX_ISIZE 65536u
#define AL_INF_LBITS 9
#define AL_INF_DBITS 6
#define AL_INF_SLACK 192u          // bits the reader may deliver past the end before a loop looks at the count

static inline const char *al_inf_strerror(int st)
{
	switch (st) {
	case AL_INF_OK: return "ok"; case AL_INF_E_HEADER: return "bad header"; case AL_INF_E_BTYPE: return "bad block type"; case AL_INF_E_STORED: return "bad stored lengths";
	case AL_INF_E_LENGTHS: return "bad code lengths"; case AL_INF_E_SYMBOL: return "bad symbol"; case AL_INF_E_DIST: return "distance too far back";
	case AL_INF_E_INPUT: return "input exhausted"; case AL_INF_E_OVER: return "output over ISIZE"; case AL_INF_E_SHORT: return "output short of ISIZE"; case AL_INF_E_CRC: return "CRC mismatch";
	}
	return "unknown";
}

AL_DHD uint32_t al_inf_le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
AL_DHD uint32_t al_inf_le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// ---- 1. the header.  m[0, avail): what is there of the member.  0: *msize = BSIZE + 1, *hdr = bytes before the deflate stream (both only from
// bytes inside avail); AL_INF_E_HEADER: not a BGZF member; -1: avail is too short to tell (the caller reads on, or calls the file truncated).
AL_DHD int al_inf_parse_header(const uint8_t *m, uint64_t avail, uint32_t *msize, uint32_t *hdr)
{
	if (avail < 12) return -1;
	if (m[0] != 0x1f || m[1] != 0x8b || m[2] != 8 || m[3] != 4) return AL_INF_E_HEADER;
	const uint32_t xlen = al_inf_le16(m + 10);
	if (avail < 12 + (uint64_t)xlen) return -1;
	uint32_t o = 0; int found = 0; uint32_t bsize = 0;
	while (o + 4 <= xlen) {                                        // (a subfield: SI1 SI2 LEN, LEN bytes; each step moves o by 4 at least)
		const uint32_t sl = al_inf_le16(m + 12 + o + 2);
		if (o + 4 + sl > xlen) return AL_INF_E_HEADER;
		if (m[12 + o] == 'B' && m[12 + o + 1] == 'C' && sl == 2 && !found) { bsize = al_inf_le16(m + 12 + o + 4); found = 1; }
		o += 4 + sl;
	}
	if (!found || o != xlen) return AL_INF_E_HEADER;
	*hdr = 12 + xlen; *msize = bsize + 1;
	if (*msize < *hdr + 1 + 8) return AL_INF_E_HEADER;            // no room for a deflate stream and the trailer
	return 0;
}

// ---- 5. the bit reader over in[0, n): values come out from the least significant bit (RFC 1951 3.1.1) --------------------------------------------
struct AlInfBits { const uint8_t *p; uint32_t n, ip; uint64_t buf; uint32_t cnt; };
AL_DHD bool al_inf_may_read(uint32_t ip, uint32_t k, uint32_t n) { return ip <= n && k <= n - ip; }        // THE predicate of every input read: bytes [ip, ip + k) lie inside
AL_DHD void al_inf_fill(AlInfBits &b)
{   // at least 57 bits in buf afterwards; zero bits where the input has ended (ip runs on, so that al_inf_used counts them)
	if (b.cnt <= 32 && al_inf_may_read(b.ip, 4, b.n)) { b.buf |= (uint64_t)al_inf_le32(b.p + b.ip) << b.cnt; b.ip += 4; b.cnt += 32; }
	while (b.cnt <= 56) { b.buf |= (uint64_t)(al_inf_may_read(b.ip, 1, b.n) ? b.p[b.ip] : 0) << b.cnt; ++b.ip; b.cnt += 8; }
}
AL_DHD void al_inf_drop(AlInfBits &b, uint32_t k) { b.buf >>= k; b.cnt -= k; }                              // k <= cnt
AL_DHD uint32_t al_inf_bits(AlInfBits &b, uint32_t k) { al_inf_fill(b); const uint32_t v = (uint32_t)(b.buf & ((1ull << k) - 1)); al_inf_drop(b, k); return v; }   // k <= 32
AL_DHD uint64_t al_inf_used(const AlInfBits &b) { return 8ull * b.ip - b.cnt; }
AL_DHD bool al_inf_over(const AlInfBits &b) { return al_inf_used(b) > 8ull * b.n; }

// ---- 3. / 4. code lengths and tables -------------------------------------------------------------------------------------------------------------------
struct AlInfTab {
	uint16_t lfast[1 << AL_INF_LBITS], dfast[1 << AL_INF_DBITS];   // length << 9 | symbol of the code that the index's low bits start with; 0: longer than the index
	uint16_t lsym[288], dsym[32];                                  // symbols in canonical order
	uint16_t lcnt[16], dcnt[16];                                   // codes per length
	uint8_t lens[320];                                             // the block's code lengths as they are read
};
enum { AL_INF_CODES = 0, AL_INF_LENS = 1, AL_INF_DISTS = 2 };
AL_DHD int al_inf_check_lengths(const uint8_t *lens, int n, int kind)
{
	int cnt[16], mx = 0, left = 1;
	for (int l = 0; l < 16; ++l) cnt[l] = 0;
	for (int s = 0; s < n; ++s) ++cnt[lens[s] & 15];
	for (int l = 1; l < 16; ++l) { left <<= 1; left -= cnt[l]; if (left < 0) return AL_INF_E_LENGTHS; if (cnt[l]) mx = l; }
	if (mx == 0) return kind == AL_INF_CODES ? AL_INF_E_LENGTHS : 0;          // (zlib builds a table of invalid entries; of the code-length alphabet nothing useful can follow)
	if (left > 0 && (kind == AL_INF_CODES || mx != 1)) return AL_INF_E_LENGTHS;
	return 0;
}
// lens[0, n), n <= 288, checked.  fast has 1 << fbits entries.
AL_DHD void al_inf_build(const uint8_t *lens, int n, uint16_t *fast, int fbits, uint16_t *cnt, uint16_t *sym)
{
	uint16_t offs[16]; uint32_t nxt[16];
	for (int l = 0; l < 16; ++l) cnt[l] = 0;
	for (int s = 0; s < n; ++s) ++cnt[lens[s] & 15];
	cnt[0] = 0; offs[1] = 0; nxt[0] = 0;
	for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + cnt[l]);
	uint32_t c = 0;
	for (int l = 1; l < 16; ++l) { c = (c + cnt[l - 1]) << 1; nxt[l] = c; }
	for (int i = 0; i < (1 << fbits); ++i) fast[i] = 0;
	for (int s = 0; s < n; ++s) {
		const int l = lens[s] & 15;
		if (!l) continue;
		sym[offs[l]++] = (uint16_t)s;
		const uint32_t code = nxt[l]++;
		if (l <= fbits) { const uint32_t r = al_dfl_rev(code, l); for (uint32_t i = r; i < (1u << fbits); i += 1u << l) fast[i] = (uint16_t)((uint32_t)l << 9 | (uint32_t)s); }
	}
}
// one symbol; -1: the next bits are no code of this set
AL_DHD int al_inf_decode(AlInfBits &b, const uint16_t *fast, int fbits, const uint16_t *cnt, const uint16_t *sym)
{
	al_inf_fill(b);
	const uint32_t e = fast[b.buf & ((1u << fbits) - 1)];
	if (e) { al_inf_drop(b, e >> 9); return (int)(e & 511); }
	int code = 0, first = 0, index = 0; uint64_t v = b.buf;
	for (int l = 1; l <= 15; ++l) {
		code |= (int)(v & 1); v >>= 1;
		const int count = cnt[l];
		if (code - count < first) { al_inf_drop(b, (uint32_t)l); return sym[index + (code - first)]; }
		index += count; first += count; first <<= 1; code <<= 1;
	}
	return -1;
}
AL_DHD void al_inf_fixed(AlInfTab *T)
{
	for (int s = 0; s < 288; ++s) T->lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
	for (int s = 0; s < 32; ++s) T->lens[288 + s] = 5;
	al_inf_build(T->lens, 288, T->lfast, AL_INF_LBITS, T->lcnt, T->lsym);
	al_inf_build(T->lens + 288, 32, T->dfast, AL_INF_DBITS, T->dcnt, T->dsym);
}

// ---- 2. tokens -------------------------------------------------------------------------------------------------------------------------------------------
#define AL_INF_TOK_MATCH  0x80000000u      // a: MATCH | length << 16 | (distance - 1)
#define AL_INF_TOK_STORED 0x40000000u      // a: STORED | length (1..65535), b: offset of the run's first byte in the deflate stream
struct AlInfState {
	AlInfBits b; uint32_t out, isize; int phase, last, err;         // phase 0: at a block header, 2: inside a Huffman block, 3: behind the final block
	uint64_t iters;                                                // loop iterations so far, all loops together
};
AL_DHD void al_inf_init(AlInfState &s, const uint8_t *in, uint32_t csize, uint32_t isize)
{
	s.b.p = in; s.b.n = csize; s.b.ip = 0; s.b.buf = 0; s.b.cnt = 0; s.out = 0; s.isize = isize; s.phase = 0; s.last = 0; s.err = 0; s.iters = 0;
}
AL_DHD bool al_inf_may_write(uint32_t out, uint32_t k, uint32_t isize) { return out <= isize && k <= isize - out; }   // THE predicate of every output write: bytes [out, out + k) lie inside
AL_DHD uint32_t al_inf_len_base(uint32_t sym) { const uint32_t e = al_dfl_len_extra(sym), k = sym - 257; return sym == 285 ? 258 : e == 0 ? 3 + k : 3 + ((4 + (k & 3)) << e); }   // sym 257..285
AL_DHD uint32_t al_inf_dist_base(uint32_t sym) { const uint32_t e = al_dfl_dist_extra(sym); return sym < 4 ? 1 + sym : 1 + ((2 + (sym & 1)) << e); }                                // sym 0..29

// the dynamic block's header: HLIT, HDIST, HCLEN, the code-length code, the lengths; the two tables are built
AL_DHD int al_inf_dynamic(AlInfState &s, AlInfTab *T)
{
	const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
	const uint32_t hd = al_inf_bits(s.b, 14);
	const int nlen = (int)(hd & 31) + 257, ndist = (int)(hd >> 5 & 31) + 1, ncode = (int)(hd >> 10 & 15) + 4;
	if (al_inf_over(s.b)) return AL_INF_E_INPUT;
	if (nlen > 286 || ndist > 30) return AL_INF_E_LENGTHS;
	uint8_t cl[19];
	for (int k = 0; k < 19; ++k) cl[k] = 0;
	for (int k = 0; k < ncode; ++k) { ++s.iters; cl[order[k]] = (uint8_t)al_inf_bits(s.b, 3); }
	if (al_inf_over(s.b)) return AL_INF_E_INPUT;
	if (al_inf_check_lengths(cl, 19, AL_INF_CODES)) return AL_INF_E_LENGTHS;
	// (the code-length code borrows the distance tables: they are built after the lengths are read)
	al_inf_build(cl, 19, T->dfast, AL_INF_DBITS, T->dcnt, T->dsym);
	int have = 0;
	while (have < nlen + ndist) {
		++s.iters;
		const int sym = al_inf_decode(s.b, T->dfast, AL_INF_DBITS, T->dcnt, T->dsym);
		if (sym < 0) return al_inf_over(s.b) ? AL_INF_E_INPUT : AL_INF_E_LENGTHS;
		int rep, val = 0;
		if (sym < 16) { rep = 1; val = sym; }
		else if (sym == 16) { if (have == 0) return AL_INF_E_LENGTHS; val = T->lens[have - 1]; rep = 3 + (int)al_inf_bits(s.b, 2); }
		else if (sym == 17) rep = 3 + (int)al_inf_bits(s.b, 3);
		else rep = 11 + (int)al_inf_bits(s.b, 7);
		if (al_inf_over(s.b)) return AL_INF_E_INPUT;
		if (have + rep > nlen + ndist) return AL_INF_E_LENGTHS;
		for (int k = 0; k < rep; ++k) T->lens[have++] = (uint8_t)val;
	}
	if (T->lens[256] == 0) return AL_INF_E_LENGTHS;
	if (al_inf_check_lengths(T->lens, nlen, AL_INF_LENS) || al_inf_check_lengths(T->lens + nlen, ndist, AL_INF_DISTS)) return AL_INF_E_LENGTHS;
	al_inf_build(T->lens, nlen, T->lfast, AL_INF_LBITS, T->lcnt, T->lsym);
	al_inf_build(T->lens + nlen, ndist, T->dfast, AL_INF_DBITS, T->dcnt, T->dsym);
	return 0;
}

// The next token: 1 with *a (and *b) set; 0 when the stream has ended behind its final block or s.err was set.
AL_DHD int al_inf_next(AlInfState &s, AlInfTab *T, uint32_t *a, uint32_t *b)
{
	for (;;) {
		++s.iters;
		if (s.err) return 0;
		if (s.phase == 0) {
			if (s.last) { s.phase = 3; return 0; }
			const uint32_t h = al_inf_bits(s.b, 3);
			if (al_inf_over(s.b)) { s.err = AL_INF_E_INPUT; return 0; }
			s.last = (int)(h & 1);
			const uint32_t type = h >> 1;
			if (type == 0) {
				al_inf_drop(s.b, s.b.cnt & 7);                                 // to the next byte boundary (used is a multiple of 8 now)
				const uint32_t w = al_inf_bits(s.b, 32);
				if (al_inf_over(s.b)) { s.err = AL_INF_E_INPUT; return 0; }
				const uint32_t len = w & 0xffff, nlen = w >> 16;
				if (len != (nlen ^ 0xffff)) { s.err = AL_INF_E_STORED; return 0; }
				const uint32_t pos = (uint32_t)(al_inf_used(s.b) >> 3);
				if (!al_inf_may_read(pos, len, s.b.n)) { s.err = AL_INF_E_INPUT; return 0; }
				if (!al_inf_may_write(s.out, len, s.isize)) { s.err = AL_INF_E_OVER; return 0; }
				s.b.ip = pos + len; s.b.buf = 0; s.b.cnt = 0;
				if (len == 0) continue;
				*a = AL_INF_TOK_STORED | len; *b = pos; s.out += len;
				return 1;
			}
			if (type == 3) { s.err = AL_INF_E_BTYPE; return 0; }
			if (type == 1) al_inf_fixed(T);
			else if ((s.err = al_inf_dynamic(s, T)) != 0) return 0;
			s.phase = 2;
			continue;
		}
		if (s.phase != 2) return 0;
		const int sym = al_inf_decode(s.b, T->lfast, AL_INF_LBITS, T->lcnt, T->lsym);
		if (sym < 0 || sym >= 286) { s.err = al_inf_over(s.b) ? AL_INF_E_INPUT : AL_INF_E_SYMBOL; return 0; }
		if (al_inf_over(s.b)) { s.err = AL_INF_E_INPUT; return 0; }
		if (sym < 256) {
			if (!al_inf_may_write(s.out, 1, s.isize)) { s.err = AL_INF_E_OVER; return 0; }
			*a = (uint32_t)sym; *b = 0; s.out += 1;
			return 1;
		}
		if (sym == 256) { s.phase = 0; continue; }
		const uint32_t len = al_inf_len_base((uint32_t)sym) + al_inf_bits(s.b, al_dfl_len_extra((uint32_t)sym));
		const int ds = al_inf_decode(s.b, T->dfast, AL_INF_DBITS, T->dcnt, T->dsym);
		if (ds < 0 || ds >= 30) { s.err = al_inf_over(s.b) ? AL_INF_E_INPUT : AL_INF_E_SYMBOL; return 0; }
		const uint32_t dist = al_inf_dist_base((uint32_t)ds) + al_inf_bits(s.b, al_dfl_dist_extra((uint32_t)ds));
		if (al_inf_over(s.b)) { s.err = AL_INF_E_INPUT; return 0; }
		if (dist > s.out) { s.err = AL_INF_E_DIST; return 0; }
		if (!al_inf_may_write(s.out, len, s.isize)) { s.err = AL_INF_E_OVER; return 0; }
		*a = AL_INF_TOK_MATCH | len << 16 | (dist - 1); *b = 0; s.out += len;
		return 1;
	}
}
// 6. behind the last token: the status of the stream (the CRC is the caller's)
AL_DHD int al_inf_finish(const AlInfState &s)
{
	if (s.err) return s.err;
	if (s.out != s.isize) return AL_INF_E_SHORT;
	if (((al_inf_used(s.b) + 7) >> 3) != s.b.n) return AL_INF_E_HEADER;      // BSIZE says the stream ends elsewhere
	return 0;
}

// ---- the members of a piece of a file, listed without inflating (host) ----------------------------------------------------------------------------------
struct AlInfMember { uint64_t in_off, out_off; uint32_t msize, isize; };
// Walks the BSIZE chain over buf[0, n) from *pos: every whole member becomes an entry (in_off relative to buf, out_off = the prefix sum of ISIZE from
// *out_n on) until the bytes end, max_out output bytes or max_mem members are reached.  *pos and *out_n are moved on.  0: stopped at a cut or a limit;
// AL_INF_E_HEADER: the bytes at *pos are no BGZF member.
template <class Vec> static inline int al_inf_list(const uint8_t *buf, uint64_t n, uint64_t *pos, uint64_t *out_n, uint64_t max_out, size_t max_mem, Vec &mem)
{
	while (*pos < n && mem.size() < max_mem) {
		uint32_t msize = 0, hdr = 0;
		const int r = al_inf_parse_header(buf + *pos, n - *pos, &msize, &hdr);
		if (r < 0) return 0;
		if (r > 0) return r;
		if (msize > n - *pos) return 0;
		const uint32_t isize = al_inf_le32(buf + *pos + msize - 4);
		if (isize > AL_INF_MAX_ISIZE) return AL_INF_E_HEADER;
		if (*out_n + isize > max_out) return 0;
		mem.push_back(AlInfMember{*pos, *out_n, msize, isize});
		*pos += msize; *out_n += isize;
	}
	return 0;
}

// ---- the host twin: the function of this file's head, evaluated serially.  m[0, msize): the member (msize from its own header); out: ISIZE bytes,
// ISIZE = the member's last four bytes, at most AL_INF_MAX_ISIZE.  Returns the status; *iters, when given, gets the loop iterations. ----------------------
static inline int al_inflate_member_host(const uint8_t *m, uint32_t msize, uint8_t *out, uint64_t *iters = nullptr)
{
	uint32_t ms = 0, hdr = 0;
	if (iters) *iters = 0;
	if (al_inf_parse_header(m, msize, &ms, &hdr) != 0 || ms != msize) return AL_INF_E_HEADER;
	const uint32_t isize = al_inf_le32(m + msize - 4), crc = al_inf_le32(m + msize - 8);
	if (isize > AL_INF_MAX_ISIZE) return AL_INF_E_HEADER;
	const uint8_t *in = m + hdr;
	AlInfTab *T = new AlInfTab;
	AlInfState s; al_inf_init(s, in, msize - hdr - 8, isize);
	uint32_t a, b, o = 0;
	while (al_inf_next(s, T, &a, &b)) {
		if (a & AL_INF_TOK_MATCH) { const uint32_t len = a >> 16 & 0x1ff, dist = (a & 0xffff) + 1; for (uint32_t j = 0; j < len; ++j) out[o + j] = out[o + j - dist]; o += len; }
		else if (a & AL_INF_TOK_STORED) { const uint32_t len = a & 0xffff; memcpy(out + o, in + b, len); o += len; }
		else out[o++] = (uint8_t)a;
	}
	delete T;
	if (iters) *iters = s.iters;
	int st = al_inf_finish(s);
	if (st == 0 && (isize ? al_dfl_crc32_host(out, isize) : 0u) != crc) st = AL_INF_E_CRC;
	return st;
}

// al_dev_deflate.h -- the BGZF block compressor of --gpu-deflate as ONE function of a block's bytes, written once for both sides: the pieces
// below are compiled for the device (k_deflate, al_deflate.hip) and for the CPU (al_deflate_block_host, the twin at the end of this file, which
// evaluates the same function serially).  The twin is what the kernel is tested against byte for byte, what tests/csrc/deflate_main.cpp runs
// under the sanitizers, and what a flush falls back to when the device refuses the staging buffers.
//
// THE FUNCTION.  Input: n bytes in[0, n), 1 <= n <= 0xff00, and a level.  Output: one gzip member (RFC 1952) with the BGZF extra field `BC`
// (SAM specification 4.1): 18 header bytes, a raw deflate stream (RFC 1951) of ONE final block, CRC32(in) and ISIZE = n.  Nothing outside
// in[0, n) is looked at, so blocks are independent of each other, of batching and of who compresses them.
//
//  1. Candidates.  A position i <= n - 4 has the hash h(i) = (le32(in + i) * 0x9E3779B1) >> 18 (14 bits).  Positions are taken in chunks of
//     AL_DFL_CHUNK = 256: cand(i) = the HIGHEST position j of an EARLIER chunk with h(j) = h(i), if there is one.  (A table slot holds the
//     maximum of what was inserted; a chunk is inserted whole after it was looked up whole.  So a position never sees its own chunk:
//     a repeat is found from the next chunk on, at a distance of up to 256 more than the nearest.)  Positions above n - 4 have no candidate.
//  2. Lengths.  len(i) = number of equal bytes of in + cand(i) and in + i, at most min(258, n - i).  Position i has the match
//     (len(i), dist = i - cand(i)) if dist <= 32768 and len(i) >= 4; otherwise it is a literal.
//  3. Parse.  Greedy from position 0: a position with a match is a match token and the parse continues at i + len(i); else a literal, i + 1.
//  4. Code.  Histograms of the 286 literal/length symbols (the end-of-block symbol counted once) and the 30 distance symbols; code lengths
//     by al_dfl_lengths (Huffman over the symbols in (frequency, symbol) order, limited to 15 bits); the distance code is completed to two
//     1-bit codes when fewer than two distance symbols are used; canonical codes (RFC 1951 3.2.2).
//  5. Form.  BFINAL = 1, BTYPE = 2, HLIT = 29, HDIST = 29, HCLEN = 15: code-length symbols 0..15 have 4-bit codes (symbol s = code s), 16/17/18
//     are unused, and the 316 code lengths follow as 4 bits each -- 1338 header bits, no run-length pass.  Then the tokens, the end-of-block
//     symbol, zero bits to the next byte.
//  6. Stored.  If level == 0, or the form of 5 would take n + 5 bytes or more, the deflate stream is one stored block instead (BTYPE = 0:
//     01, LEN, NLEN, the n bytes): the member is n + 31 bytes and never more, which keeps it within the 65536 a BGZF block may have.
//
// Every step is a pure function of in[0, n): where lanes meet on the device (table slots, histogram counters, words of the bit stream) they
// do so through max, + and OR, whose results do not depend on the order of arrival.
#pragma once
#include <stdint.h>
#include <string.h>
#if defined(__HIPCC__)
#define AL_DHD __host__ __device__ inline
#else
#define AL_DHD static inline
#endif

#define AL_DFL_BLOCK   0xff00u      // uncompressed bytes of a full BGZF block
#define AL_DFL_SLOT    65536u       // largest member
#define AL_DFL_CHUNK   256u
#define AL_DFL_HBITS   14
#define AL_DFL_NLIT    286
#define AL_DFL_NDIST   30
#define AL_DFL_HDRBITS (3 + 5 + 5 + 4 + 19 * 3 + (AL_DFL_NLIT + AL_DFL_NDIST) * 4)
#define AL_DFL_POLY    0xedb88320u

AL_DHD uint32_t al_dfl_hash(uint32_t w) { return (w * 0x9E3779B1u) >> (32 - AL_DFL_HBITS); }
AL_DHD int al_dfl_log2(uint32_t x) { int r = 0; while (x >>= 1) ++r; return r; }       // x >= 1
AL_DHD uint32_t al_dfl_rev(uint32_t c, int n) { uint32_t r = 0; for (int i = 0; i < n; ++i) { r = r << 1 | (c & 1); c >>= 1; } return r; }

// length 3..258 -> symbol 257..285, number and value of its extra bits (RFC 1951 3.2.5)
AL_DHD void al_dfl_len_sym(uint32_t len, uint32_t *sym, uint32_t *eb, uint32_t *ev)
{
	const uint32_t l = len - 3;
	if (len == 258) { *sym = 285; *eb = 0; *ev = 0; }
	else if (l < 8) { *sym = 257 + l; *eb = 0; *ev = 0; }
	else { const uint32_t e = (uint32_t)al_dfl_log2(l) - 2; *sym = 257 + 4 * (e + 1) + ((l >> e) & 3); *eb = e; *ev = l & ((1u << e) - 1); }
}
// distance 1..32768 -> symbol 0..29
AL_DHD void al_dfl_dist_sym(uint32_t dist, uint32_t *sym, uint32_t *eb, uint32_t *ev)
{
	const uint32_t d = dist - 1;
	if (d < 4) { *sym = d; *eb = 0; *ev = 0; }
	else { const uint32_t hb = (uint32_t)al_dfl_log2(d), e = hb - 1; *sym = 2 * hb + ((d >> e) & 1); *eb = e; *ev = d & ((1u << e) - 1); }
}
AL_DHD uint32_t al_dfl_len_extra(uint32_t sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }     // extra bits of a length symbol
AL_DHD uint32_t al_dfl_dist_extra(uint32_t sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }

// Code lengths of the `nu` used symbols, given in ascending (frequency, symbol) order: A[k] = frequency, S[k] = symbol.  Huffman by the in-place
// method of Moffat and Katajainen (1995), then limited to 15 bits by moving codes between lengths until the Kraft sum is 1 again, the more frequent
// symbol getting the shorter code.  len[] must be zero on entry.  One used symbol gets a 1-bit code.
AL_DHD void al_dfl_lengths_sorted(uint32_t *A, const uint16_t *S, int nu, uint8_t *len)
{
	if (nu <= 0) return;
	if (nu == 1) { len[S[0]] = 1; return; }
	int root = 0, leaf = 2, next;
	A[0] += A[1];
	for (next = 1; next < nu - 1; ++next) {
		if (leaf >= nu || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; } else A[next] = A[leaf++];
		if (leaf >= nu || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; } else A[next] += A[leaf++];
	}
	A[nu - 2] = 0;
	for (next = nu - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
	int avbl = 1, used = 0, dpth = 0;
	root = nu - 2; next = nu - 1;
	while (avbl > 0) {
		while (root >= 0 && (int)A[root] == dpth) { ++used; --root; }
		while (avbl > used) { A[next--] = (uint32_t)dpth; --avbl; }
		avbl = 2 * used; ++dpth; used = 0;
	}
	// A[k] = depth of the k-th least frequent symbol (non-increasing in k)
	uint32_t num[16]; uint32_t total = 0;
	for (int l = 0; l < 16; ++l) num[l] = 0;
	for (int k = 0; k < nu; ++k) ++num[A[k] > 15 ? 15 : A[k]];
	for (int l = 1; l <= 15; ++l) total += num[l] << (15 - l);
	while (total > (1u << 15)) {
		--num[15];
		for (int l = 14; l >= 1; --l) if (num[l]) { --num[l]; num[l + 1] += 2; break; }
		--total;
	}
	int k = nu;
	for (int l = 1; l <= 15; ++l) for (uint32_t c = 0; c < num[l]; ++c) len[S[--k]] = (uint8_t)l;
}
// The same from a histogram: orders the used symbols (serially) and calls the above.  A: n words, S: n halfwords of scratch.
AL_DHD void al_dfl_lengths(const uint32_t *freq, int n, uint8_t *len, uint32_t *A, uint16_t *S)
{
	int nu = 0;
	for (int s = 0; s < n; ++s) {
		len[s] = 0;
		if (!freq[s]) continue;
		int k = nu++;
		while (k > 0 && A[k - 1] > freq[s]) { A[k] = A[k - 1]; S[k] = S[k - 1]; --k; }     // (symbols come in ascending order: equal frequencies stay in symbol order)
		A[k] = freq[s]; S[k] = (uint16_t)s;
	}
	al_dfl_lengths_sorted(A, S, nu, len);
}
// the distance code as it is sent: at least two codes, so that every inflater takes it as complete
AL_DHD void al_dfl_fix_dist(uint8_t *dlen)
{
	int nu = 0, s0 = -1;
	for (int s = 0; s < AL_DFL_NDIST; ++s) if (dlen[s]) { ++nu; s0 = s; }
	if (nu == 0) dlen[0] = dlen[1] = 1;
	else if (nu == 1) dlen[s0 == 0 ? 1 : 0] = 1;
}
// canonical codes (RFC 1951 3.2.2), stored bit-reversed: a deflate stream takes Huffman codes from their most significant bit
AL_DHD void al_dfl_codes(const uint8_t *len, int n, uint16_t *code)
{
	uint32_t cnt[16], nxt[16];
	for (int l = 0; l < 16; ++l) cnt[l] = 0;
	for (int s = 0; s < n; ++s) ++cnt[len[s]];
	cnt[0] = 0; nxt[0] = 0;
	uint32_t c = 0;
	for (int l = 1; l < 16; ++l) { c = (c + cnt[l - 1]) << 1; nxt[l] = c; }
	for (int s = 0; s < n; ++s) code[s] = len[s] ? (uint16_t)al_dfl_rev(nxt[len[s]]++, len[s]) : 0;
}

// ---- the bit stream: values go in from the least significant bit (RFC 1951 3.1.1); a sink ORs a 32-bit value into word w --------------------
template <class Sink> AL_DHD void al_dfl_put(Sink &s, uint64_t bitpos, uint64_t val, uint32_t nbits)
{   // val < 2^nbits, nbits <= 48
	if (!nbits) return;
	const uint32_t w = (uint32_t)(bitpos >> 5), sh = (uint32_t)(bitpos & 31);
	s.orw(w, (uint32_t)(val << sh));
	const uint64_t hi = sh ? val >> (32 - sh) : val >> 32;
	if (sh + nbits > 32) s.orw(w + 1, (uint32_t)hi);
	if (sh + nbits > 64) s.orw(w + 2, (uint32_t)(hi >> 32));
}
// the dynamic block's header at bit b0, written by `nl` cooperating callers (caller `lane` of them; a serial caller passes 0, 1)
template <class Sink> AL_DHD void al_dfl_header(Sink &s, uint64_t b0, uint32_t lane, uint32_t nl, const uint8_t *llen, const uint8_t *dlen)
{
	if (lane == 0) {
		al_dfl_put(s, b0, 1u | 2u << 1 | (uint32_t)(AL_DFL_NLIT - 257) << 3 | (uint32_t)(AL_DFL_NDIST - 1) << 8 | 15u << 13, 17);
		// code lengths of the code-length code in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15: three zeros, then sixteen fours
		uint64_t v = 0;
		for (int k = 3; k < 19; ++k) v |= (uint64_t)4 << (3 * k);
		al_dfl_put(s, b0 + 17, v & 0xffffffffull, 32); al_dfl_put(s, b0 + 49, v >> 32, 25);
	}
	for (uint32_t k = lane; k < AL_DFL_NLIT + AL_DFL_NDIST; k += nl) {
		const uint32_t l = k < AL_DFL_NLIT ? llen[k] : dlen[k - AL_DFL_NLIT];
		al_dfl_put(s, b0 + 74 + 4 * (uint64_t)k, al_dfl_rev(l, 4), 4);
	}
}
// one token as bits: m = 0 for the literal `lit`, else len << 16 | (dist - 1)
AL_DHD uint64_t al_dfl_token(uint32_t m, uint32_t lit, const uint16_t *lcode, const uint8_t *llen, const uint16_t *dcode, const uint8_t *dlen, uint32_t *nbits)
{
	if (!m) { *nbits = llen[lit]; return lcode[lit]; }
	uint32_t ls, le, lv, ds, de, dv;
	al_dfl_len_sym(m >> 16, &ls, &le, &lv); al_dfl_dist_sym((m & 0xffff) + 1, &ds, &de, &dv);
	uint64_t v = lcode[ls]; uint32_t nb = llen[ls];
	v |= (uint64_t)lv << nb; nb += le;
	v |= (uint64_t)dcode[ds] << nb; nb += dlen[ds];
	v |= (uint64_t)dv << nb; nb += de;
	*nbits = nb; return v;
}

// ---- CRC32 (the gzip one, reflected, polynomial 0xedb88320) by parts ------------------------------------------------------------------------
// A part's register starts at 0 (at 0xffffffff for the part that holds the first byte) and is run over the part's bytes; the register of a
// concatenation is reg(A) * x^(8 |B|) + reg(B) in GF(2)[x] / P; the CRC is the whole's register, inverted.
AL_DHD uint32_t al_dfl_crc_byte(uint32_t r, uint8_t b) { r ^= b; for (int k = 0; k < 8; ++k) r = (r >> 1) ^ (AL_DFL_POLY & (0u - (r & 1))); return r; }
AL_DHD uint32_t al_dfl_crc_mul(uint32_t a, uint32_t b)
{   // product of two residues, reflected: bit 31 is x^0
	uint32_t p = 0;
	for (int k = 0; k < 32; ++k) { if (a & (0x80000000u >> k)) p ^= b; b = (b >> 1) ^ (AL_DFL_POLY & (0u - (b & 1))); }
	return p;
}
AL_DHD uint32_t al_dfl_crc_xpow8(uint64_t nbytes)
{   // x^(8 nbytes) mod P
	uint32_t r = 0x80000000u, sq = 0x00800000u;       // x^0, x^8
	for (; nbytes; nbytes >>= 1) { if (nbytes & 1) r = al_dfl_crc_mul(r, sq); sq = al_dfl_crc_mul(sq, sq); }
	return r;
}
AL_DHD uint32_t al_dfl_crc_join(uint32_t reg_a, uint32_t reg_b, uint64_t len_b) { return al_dfl_crc_mul(reg_a, al_dfl_crc_xpow8(len_b)) ^ reg_b; }

// ---- the member around the deflate stream ------------------------------------------------------------------------------------------------------
AL_DHD void al_dfl_member_header(uint8_t *h, uint32_t total)
{
	const uint8_t t[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
	for (int k = 0; k < 16; ++k) h[k] = t[k];
	h[16] = (uint8_t)((total - 1) & 0xff); h[17] = (uint8_t)((total - 1) >> 8);
}

// ---- the host twin: the function of this file's head, evaluated serially.  dst holds AL_DFL_SLOT bytes; returns the member's size. -------------
struct AlDflHostSink { uint32_t *w; void orw(uint32_t i, uint32_t v) { w[i] |= v; } };
static inline uint32_t al_dfl_le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
static inline uint32_t al_dfl_crc32_host(const uint8_t *p, size_t n)
{   // by parts of 64 bytes, joined: the form the kernel computes
	uint32_t reg = 0;
	for (size_t o = 0; o < n; o += 64) {
		const size_t m = n - o < 64 ? n - o : 64;
		uint32_t r = o == 0 ? 0xffffffffu : 0;
		for (size_t k = 0; k < m; ++k) r = al_dfl_crc_byte(r, p[o + k]);
		reg = o == 0 ? r : al_dfl_crc_join(reg, r, m);
	}
	return ~reg;
}
// hist, when given, gets the token histograms of the parse: 286 literal/length counts, then 30 distance counts (zeros for level 0).
static inline uint32_t al_deflate_block_host(const uint8_t *in, uint32_t n, int level, uint8_t *dst, int *stored, uint32_t *hist = nullptr)
{
	static const uint32_t NW = AL_DFL_SLOT / 4;
	uint32_t *m = new uint32_t[AL_DFL_BLOCK], *tab = new uint32_t[1u << AL_DFL_HBITS](), *outw = new uint32_t[NW + 4]();
	uint32_t lfreq[AL_DFL_NLIT] = {0}, dfreq[AL_DFL_NDIST] = {0}, A[AL_DFL_NLIT];
	uint16_t S[AL_DFL_NLIT], lcode[AL_DFL_NLIT], dcode[AL_DFL_NDIST]; uint8_t llen[AL_DFL_NLIT], dlen[AL_DFL_NDIST];
	bool huff = level != 0; uint32_t comp = 0;
	if (huff) {
		const uint32_t nh = n >= 4 ? n - 3 : 0;
		for (uint32_t base = 0; base < nh; base += AL_DFL_CHUNK) {
			const uint32_t end = base + AL_DFL_CHUNK < nh ? base + AL_DFL_CHUNK : nh;
			for (uint32_t i = base; i < end; ++i) m[i] = tab[al_dfl_hash(al_dfl_le32(in + i))];
			for (uint32_t i = base; i < end; ++i) { uint32_t &t = tab[al_dfl_hash(al_dfl_le32(in + i))]; if (i + 1 > t) t = i + 1; }
		}
		for (uint32_t i = 0; i < n; ++i) {
			const uint32_t c = i < nh ? m[i] : 0; uint32_t l = 0;
			if (c && i - (c - 1) <= 32768) { const uint32_t cap = n - i < 258 ? n - i : 258; const uint8_t *a = in + (c - 1), *b = in + i; while (l < cap && a[l] == b[l]) ++l; }
			m[i] = l >= 4 ? l << 16 | (i - (c - 1) - 1) : 0;
		}
		for (uint32_t i = 0; i < n; ) {
			if (m[i]) { uint32_t s, e, v; al_dfl_len_sym(m[i] >> 16, &s, &e, &v); ++lfreq[s]; al_dfl_dist_sym((m[i] & 0xffff) + 1, &s, &e, &v); ++dfreq[s]; i += m[i] >> 16; }
			else { ++lfreq[in[i]]; ++i; }
		}
		++lfreq[256];
		al_dfl_lengths(lfreq, AL_DFL_NLIT, llen, A, S); al_dfl_lengths(dfreq, AL_DFL_NDIST, dlen, A, S); al_dfl_fix_dist(dlen);
		al_dfl_codes(llen, AL_DFL_NLIT, lcode); al_dfl_codes(dlen, AL_DFL_NDIST, dcode);
		uint64_t bits = AL_DFL_HDRBITS;
		for (int s = 0; s < AL_DFL_NLIT; ++s) bits += (uint64_t)lfreq[s] * (llen[s] + (s > 256 ? al_dfl_len_extra((uint32_t)s) : 0));
		for (int s = 0; s < AL_DFL_NDIST; ++s) bits += (uint64_t)dfreq[s] * (dlen[s] + al_dfl_dist_extra((uint32_t)s));
		comp = (uint32_t)((bits + 7) >> 3);
		if (comp >= n + 5) huff = false;
	}
	uint32_t total;
	uint8_t *ob = (uint8_t *)outw;            // (little-endian hosts: the words are the stream's bytes)
	if (huff) {
		AlDflHostSink sk{outw};
		uint64_t bp = 18 * 8;
		al_dfl_header(sk, bp, 0, 1, llen, dlen); bp += AL_DFL_HDRBITS;
		for (uint32_t i = 0; i < n; ) {
			uint32_t nb; const uint64_t v = al_dfl_token(m[i], in[i], lcode, llen, dcode, dlen, &nb);
			al_dfl_put(sk, bp, v, nb); bp += nb;
			i += m[i] ? m[i] >> 16 : 1;
		}
		al_dfl_put(sk, bp, lcode[256], llen[256]);
		total = 18 + comp + 8;
	} else {
		ob[18] = 1; ob[19] = (uint8_t)(n & 0xff); ob[20] = (uint8_t)(n >> 8); ob[21] = (uint8_t)(~n & 0xff); ob[22] = (uint8_t)((~n >> 8) & 0xff);
		memcpy(ob + 23, in, n);
		total = 18 + 5 + n + 8;
	}
	al_dfl_member_header(ob, total);
	const uint32_t crc = al_dfl_crc32_host(in, n);
	for (int k = 0; k < 4; ++k) { ob[total - 8 + k] = (uint8_t)(crc >> (8 * k)); ob[total - 4 + k] = (uint8_t)(n >> (8 * k)); }
	memcpy(dst, ob, total);
	if (stored) *stored = huff ? 0 : 1;
	if (hist) { for (int s = 0; s < AL_DFL_NLIT; ++s) hist[s] = lfreq[s]; for (int s = 0; s < AL_DFL_NDIST; ++s) hist[AL_DFL_NLIT + s] = dfreq[s]; }
	delete[] m; delete[] tab; delete[] outw;
	return total;
}

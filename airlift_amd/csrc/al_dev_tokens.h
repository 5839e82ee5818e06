// al_dev_tokens.h -- the tokens of `tokens --gaps-bed` as ONE function of a table of regions, written once for both sides: the pieces below are compiled for
// the device (k_tok_setup, al_tokens.hip) and for the CPU (the twin at the end of this file, which evaluates the same function serially).  The twin is what
// the kernel is tested against, and what tests/csrc/tokens_main.cpp runs under the sanitizers.
//
// THE FUNCTION.  A BED row "name \t a \t b" stands for what `samtools faidx REF name:a-b` prints (extract_fasta_regions_with_bedfile.sh:4-7 hands the BED
// numbers to that 1-based inclusive parser, and a = 0 reads as a = 1): the header ">name:a-b" from the literal text of the three fields, the sequence the
// contig's bases [max(a, 1) - 1, min(b, contig length)).  Region r of the table is one row:
//
//   src[r]        first base of the region in the index's concatenated 4-bit reference: seq_off[contig] + max(a, 1) - 1
//   len[r]        its length
//   first_tok[r]  exclusive prefix sum of the token counts; first_tok[n_rows] = all tokens
//   h_prefix[r]   the X31 state (khash.h:383-389) after the bytes "name:a-b_"
//
// Tokens of a region (gaps_to_fasta.py's range(R, len, S)): k = 0, 1, ... while k * S + R < len -- al_tok_count.  Token t of the run belongs to the LAST
// row whose first_tok is <= t (rows without tokens make equal neighbours; the last of them owns the token) -- al_tok_row.  Its k is t - first_tok[row], its
// window starts at src[row] + k * S, its name is "name:a-b_<k * S>", and its fragment hash (map.c:291-293) continues h_prefix over the decimal digits of
// k * S and is finished with the two Wang terms -- al_tok_hash.
#pragma once
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "al_dev_deflate.h"       // AL_DHD

// tokens of a region of `len` bases: k = 0, 1, ... while k * S + R < len
AL_DHD uint64_t al_tok_count(uint32_t len, uint32_t R, uint32_t S) { return len > R ? (uint64_t)(len - R - 1) / S + 1 : 0; }

AL_DHD uint32_t al_tok_wang(uint32_t key)
{   // khash.h:398-408
	key += ~(key << 15); key ^= (key >> 10); key += (key << 3); key ^= (key >> 6); key += ~(key << 11); key ^= (key >> 16);
	return key;
}
// the X31 state h (of a non-empty prefix) continued over the decimal digits of off, most significant first
AL_DHD uint32_t al_tok_x31_digits(uint32_t h, uint32_t off)
{
	uint32_t p = 1;
	while (off / p >= 10) p *= 10;                                       // (off / p: no overflow of p at 4 294 967 295)
	for (; p; p /= 10) h = (h << 5) - h + (uint32_t)('0' + off / p % 10);
	return h;
}
AL_DHD uint32_t al_tok_hash(uint32_t h_prefix, uint32_t off, int qlen, int seed)
{
	uint32_t h = al_tok_x31_digits(h_prefix, off);
	h ^= al_tok_wang((uint32_t)qlen) + al_tok_wang((uint32_t)seed);
	return al_tok_wang(h);
}
// the row that owns token t: the last one with first_tok <= t (first_tok has n_rows + 1 entries, t < first_tok[n_rows])
AL_DHD uint32_t al_tok_row(const uint64_t *first_tok, uint32_t n_rows, uint64_t t)
{
	uint32_t lo = 0, hi = n_rows;                                        // first_tok[lo] <= t < first_tok[hi]
	while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (first_tok[mid] <= t) lo = mid; else hi = mid; }
	return lo;
}
struct AlTokTab { const uint64_t *first_tok, *src; const uint32_t *h_prefix; uint32_t n_rows; };
// token t: its row, the first base of its window, its fragment hash
AL_DHD void al_tok_setup(const AlTokTab &T, uint64_t t, int R, int S, int seed, uint32_t *row, uint64_t *start, uint32_t *hash)
{
	const uint32_t r = al_tok_row(T.first_tok, T.n_rows, t);
	const uint32_t off = (uint32_t)(t - T.first_tok[r]) * (uint32_t)S;   // below len[r]: 32 bits
	*row = r; *start = T.src[r] + off; *hash = al_tok_hash(T.h_prefix[r], off, R, seed);
}

// ---- the host side: BED rows, the table, the twin ----------------------------------------------------------------------------------------------------------------
static inline uint32_t al_tok_x31(const char *s, size_t l)
{   // khash.h:383-389 over l bytes (none of them NUL)
	uint32_t h = 0;
	if (l) { h = (uint32_t)(unsigned char)s[0]; for (size_t i = 1; i < l; ++i) h = (h << 5) - h + (uint32_t)(unsigned char)s[i]; }
	return h;
}

struct AlTokRow { std::string head; uint32_t rid = 0, start = 0, len = 0; };      // head: "name:a-b", the region [start, start + len) of contig rid

// One BED line (without its newline) -> row.  0: a row; 1: an empty line; -1: refused, *why says it.  contig(name, len_out) gives the contig's index or -1.
template <class F>
static inline int al_tok_parse_row(const char *l, size_t n, F contig, AlTokRow &row, const char **why)
{
	while (n && (l[n - 1] == '\n' || l[n - 1] == '\r')) --n;
	if (n == 0) return 1;
	size_t f[4]; int nf = 0; f[nf++] = 0;                                 // field i is [f[i], f[i + 1] - 1)
	for (size_t i = 0; i < n && nf < 4; ++i) if (l[i] == '\t') f[nf++] = i + 1;
	if (nf < 3) { *why = "fewer than three tab-separated fields"; return -1; }
	if (nf < 4) f[3] = n + 1;
	uint64_t v[2];
	for (int j = 0; j < 2; ++j) {
		const size_t a = f[j + 1], b = f[j + 2] - 1;
		if (a >= b) { *why = j ? "the end is not a number" : "the start is not a number"; return -1; }
		uint64_t x = 0;
		for (size_t i = a; i < b; ++i) {
			if (l[i] < '0' || l[i] > '9') { *why = j ? "the end is not a number" : "the start is not a number"; return -1; }
			x = x * 10 + (uint64_t)(l[i] - '0'); if (x > (1ull << 40)) x = 1ull << 40;      // (far above any contig: clamped like every end beyond one)
		}
		v[j] = x;
	}
	if (v[1] < v[0]) { *why = "the end lies before the start"; return -1; }
	const std::string name(l, f[1] - 1);
	uint32_t clen = 0; const int64_t rid = contig(name, &clen);
	if (rid < 0) { *why = "the reference has no contig of this name"; return -1; }
	const uint64_t s0 = (v[0] ? v[0] : 1) - 1, e0 = v[1] < clen ? v[1] : clen;
	row.head.assign(l, f[1] - 1); row.head += ':'; row.head.append(l + f[1], f[2] - 1 - f[1]); row.head += '-'; row.head.append(l + f[2], f[3] - 1 - f[2]);
	row.rid = (uint32_t)rid; row.start = (uint32_t)(s0 < e0 ? s0 : e0); row.len = (uint32_t)(s0 < e0 ? e0 - s0 : 0);
	return 0;
}

// first_tok (n + 1 entries) and h_prefix (n) of n regions with the heads `heads` and lengths `len`
static inline void al_tok_table(const std::vector<std::string> &heads, const uint32_t *len, int R, int S, std::vector<uint64_t> &first_tok, std::vector<uint32_t> &h_prefix)
{
	const size_t n = heads.size();
	first_tok.assign(n + 1, 0); h_prefix.assign(n, 0);
	for (size_t i = 0; i < n; ++i) {
		first_tok[i + 1] = first_tok[i] + al_tok_count(len[i], (uint32_t)R, (uint32_t)S);
		const uint32_t h = al_tok_x31(heads[i].data(), heads[i].size());
		h_prefix[i] = (h << 5) - h + (uint32_t)'_';
	}
}
// the twin of k_tok_setup: tokens [t0, t0 + n)
static inline void al_tok_setup_host(const AlTokTab &T, uint64_t t0, uint64_t n, int R, int S, int seed, uint64_t *start, uint32_t *hash)
{
	for (uint64_t i = 0; i < n; ++i) { uint32_t row; al_tok_setup(T, t0 + i, R, S, seed, &row, start + i, hash + i); }
}
// the runs (first token relative to t0, row) of tokens [t0, t0 + n), n > 0: what al_regions_groups takes, in closed form from first_tok
static inline void al_tok_runs(const uint64_t *first_tok, uint32_t n_rows, uint64_t t0, uint64_t n, std::vector<uint32_t> &g_first, std::vector<uint32_t> &g_id)
{
	g_first.clear(); g_id.clear();
	uint32_t r = al_tok_row(first_tok, n_rows, t0);
	g_first.push_back(0); g_id.push_back(r);
	for (++r; r < n_rows && first_tok[r] < t0 + n; ++r)
		if (first_tok[r + 1] > first_tok[r]) { g_first.push_back((uint32_t)(first_tok[r] - t0)); g_id.push_back(r); }
}
// name and bases of one token as the SAM sink prints them: "head_<off>", and upper-case ACGTN from the 4-bit reference
static inline void al_tok_name(const std::string &head, uint32_t off, std::string &o) { char num[16]; o = head; o.append(num, (size_t)snprintf(num, sizeof(num), "_%u", off)); }
static inline void al_tok_bases(const uint32_t *S4, uint64_t start, int R, char *o)
{
	for (int j = 0; j < R; ++j) { const uint64_t p = start + (uint64_t)j; const uint32_t c = S4[p >> 3] >> ((p & 7) << 2) & 15u; o[j] = c < 4 ? "ACGT"[c] : 'N'; }
}

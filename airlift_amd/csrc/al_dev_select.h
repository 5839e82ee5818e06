// al_dev_select.h -- the read selection of --gpu-select (extract-sequence, remap) as ONE function of a FASTQ text and a set of names, written once for
// both sides: the pieces below are compiled for the device (k_fq_select / k_fq_gather, al_select.hip) and for the CPU (the twin at the end of this file,
// which evaluates the same function record by record).  The twin is what the kernels are tested against byte for byte, what runs where there is no
// device, and what tests/csrc/select_main.cpp runs under the sanitizers.
//
// THE FUNCTION.  Input: a text of complete lines, its strict four-line records as k_fq_parse (al_stream.hip) delivers them (AlFqRec: name, sequence and
// quality as offsets into the text), and the set of selected names.  Output per record: 1 when its name is in the set, else 0; `first_bad`, the first
// record the default reader (AlSeqReader, kseq grammar) may read differently; and for the selected records in front of first_bad a compact arena --
// name, sequence, quality, one record behind the other in file order -- with one descriptor each.
//
//  1. Hash.  al_sel_hash: FNV-1a over the name bytes, 64 bits, finished with a multiply-shift mix so that the table index (low bits) and the tag (high
//     32 bits) both depend on every byte.
//  2. Probe.  al_sel_probe: an open-addressing table of 2^k slots, at most half of them in use, linear probing from hash & mask.  A slot holds offset and
//     length of a name in the name arena and the tag (never 0: 0 marks a free slot).  Tag and length are compared first, then the bytes: a hit is a
//     hit only when the bytes are equal, so the answer is exact whatever the hash does.  The loop is capped at the table's size.
//  3. Grammar.  al_sel_irregular: a strict record whose sequence line is not empty and starts with '>', '+' or '@' -- the default reader ends a
//     sequence at a line that starts so, and reads such a record differently.  It lowers first_bad like any record k_fq_parse refuses.
//  4. Bytes.  A selected record takes name_len + 2 * len bytes of the arena (al_sel_bytes); its sequence bytes u / U become t / T (al_sel_base,
//     bseq.c:72-74), everything else is copied as it is.  Line ends ('\n', a trailing '\r') are outside the lengths k_fq_parse measures.
#pragma once
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include "al_dev_deflate.h"       // AL_DHD

struct AlFqRec { uint32_t name, name_len, seq, len, qual; };      // one FASTQ record: offsets into its file's text (k_fq_parse)
struct AlSelSlot { uint32_t off, len, tag; };                     // tag 0: free
struct AlSelTable { const AlSelSlot *slot; const uint8_t *names; uint32_t mask; };   // mask + 1 slots
struct AlSelDesc { uint32_t off, name_len, len; };                // a selected record in the arena: name at off, sequence at off + name_len, quality at off + name_len + len

AL_DHD uint64_t al_sel_hash(const uint8_t *s, uint32_t l)
{
	uint64_t h = 0xcbf29ce484222325ull;
	for (uint32_t i = 0; i < l; ++i) { h ^= s[i]; h *= 0x100000001b3ull; }
	h ^= h >> 32; h *= 0x9e3779b97f4a7c15ull; h ^= h >> 29;
	return h;
}
AL_DHD uint32_t al_sel_tag(uint64_t h) { const uint32_t t = (uint32_t)(h >> 32); return t ? t : 1u; }
AL_DHD bool al_sel_probe(const AlSelTable &T, const uint8_t *s, uint32_t l)
{
	const uint64_t h = al_sel_hash(s, l);
	const uint32_t tag = al_sel_tag(h);
	uint32_t i = (uint32_t)h & T.mask;
	for (uint32_t step = 0; step <= T.mask; ++step, i = (i + 1) & T.mask) {
		const AlSelSlot e = T.slot[i];
		if (e.tag == 0) return false;
		if (e.tag != tag || e.len != l) continue;
		uint32_t j = 0;
		while (j < l && T.names[e.off + j] == s[j]) ++j;
		if (j == l) return true;
	}
	return false;
}
AL_DHD bool al_sel_irregular(const uint8_t *t, const AlFqRec &r) { return r.len != 0 && (t[r.seq] == '>' || t[r.seq] == '+' || t[r.seq] == '@'); }
AL_DHD uint32_t al_sel_bytes(const AlFqRec &r) { return r.name_len + 2 * r.len; }
AL_DHD uint8_t al_sel_base(uint8_t c) { return (c == 'u' || c == 'U') ? (uint8_t)(c - 1) : c; }

// ---- the table's builder (host) ----------------------------------------------------------------------------------------------------------------------------
struct AlSelNames {
	std::vector<AlSelSlot> slot; std::vector<uint8_t> names;
	AlSelTable table() const { return AlSelTable{slot.data(), names.data(), (uint32_t)slot.size() - 1}; }
};
// names: any range of std::string without duplicates.  2^k slots with 2^k >= 2 n (and at least 2): at most half in use, so every probe ends at a free slot.
template <class Set> static inline int al_sel_build(const Set &set, AlSelNames &N)
{
	size_t n = 0, bytes = 0;
	for (const std::string &s : set) { ++n; bytes += s.size(); }
	if (n >= (1u << 30) || bytes >= (1ull << 32)) return -1;
	size_t cap = 2; while (cap < 2 * n) cap <<= 1;
	N.slot.assign(cap, AlSelSlot{0, 0, 0}); N.names.clear(); N.names.reserve(bytes + 1);
	const uint32_t mask = (uint32_t)cap - 1;
	for (const std::string &s : set) {
		const uint64_t h = al_sel_hash((const uint8_t *)s.data(), (uint32_t)s.size());
		uint32_t i = (uint32_t)h & mask;
		while (N.slot[i].tag) i = (i + 1) & mask;
		N.slot[i] = AlSelSlot{(uint32_t)N.names.size(), (uint32_t)s.size(), al_sel_tag(h)};
		N.names.insert(N.names.end(), s.begin(), s.end());
	}
	N.names.push_back(0);                                        // (never empty: the device copy has a byte to point at)
	return 0;
}

// ---- the host twin ---------------------------------------------------------------------------------------------------------------------------------------------
// Line index and strict-record test of t[0, n), as k_nl_fill / k_fq_parse compute them: ls[j] = offset of line j, ls[lines] = end of the complete lines.
static inline void al_sel_lines_host(const uint8_t *t, uint64_t n, std::vector<uint32_t> &ls)
{
	ls.clear(); ls.push_back(0);
	for (const uint8_t *p = t, *e = t + n; p < e; ) { const uint8_t *q = (const uint8_t *)memchr(p, '\n', (size_t)(e - p)); if (!q) break; ls.push_back((uint32_t)(q - t) + 1); p = q + 1; }
}
static inline bool al_sel_ws(uint8_t c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f'; }
static inline bool al_sel_parse_host(const uint8_t *t, const uint32_t *ls, uint32_t r, AlFqRec &o)
{
	const uint32_t p0 = ls[4 * r], p1 = ls[4 * r + 1], p2 = ls[4 * r + 2], p3 = ls[4 * r + 3], p4 = ls[4 * r + 4];
	bool ok = t[p0] == '@' && t[p2] == '+';
	uint32_t s1 = p2 - 1, q1 = p4 - 1;
	if (s1 > p1 && t[s1 - 1] == '\r') --s1;
	if (q1 > p3 && t[q1 - 1] == '\r') --q1;
	if (s1 - p1 != q1 - p3) ok = false;
	uint32_t e = p0 + 1; const uint32_t le = p1 - 1;
	while (e < le && !al_sel_ws(t[e])) ++e;
	o.name = p0 + 1; o.name_len = e - (p0 + 1); o.seq = p1; o.len = s1 - p1; o.qual = p3;
	return ok;
}
// What k_fq_select computes for the n_rec records of a parsed text: flag[r], bytes[r] (0 when not selected); returns the first irregular record (~0: none).
static inline uint64_t al_sel_select_host(const uint8_t *t, const AlFqRec *rec, uint32_t n_rec, const AlSelTable &T, uint32_t *flag, uint32_t *bytes)
{
	uint64_t bad = ~0ull;
	for (uint32_t r = 0; r < n_rec; ++r) {
		const bool sel = al_sel_probe(T, t + rec[r].name, rec[r].name_len);
		flag[r] = sel ? 1u : 0u; bytes[r] = sel ? al_sel_bytes(rec[r]) : 0u;
		if (bad == ~0ull && al_sel_irregular(t, rec[r])) bad = r;
	}
	return bad;
}
// What k_fq_gather writes for records [0, n): desc[k] and the arena bytes of the k-th selected record, at the exclusive sums of flag / bytes.
static inline void al_sel_gather_host(const uint8_t *t, const AlFqRec *rec, uint32_t n, const uint32_t *flag, AlSelDesc *desc, uint8_t *arena)
{
	uint32_t k = 0, off = 0;
	for (uint32_t r = 0; r < n; ++r) {
		if (!flag[r]) continue;
		const AlFqRec &q = rec[r];
		desc[k++] = AlSelDesc{off, q.name_len, q.len};
		memcpy(arena + off, t + q.name, q.name_len); off += q.name_len;
		for (uint32_t j = 0; j < q.len; ++j) arena[off + j] = al_sel_base(t[q.seq + j]);
		off += q.len;
		memcpy(arena + off, t + q.qual, q.len); off += q.len;
	}
}

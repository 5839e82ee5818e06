// al_dev_lift.h -- `lift`: the reads of a BAM that lie in constant regions moved across the chain file (run_pipeline.sh:92-95, FastRemap) as ONE function of
// the BAM's records and the chain file's block table, written once for both sides: the pieces below are compiled for the device (k_bam_walk, k_lift,
// k_lift_gather: al_lift.hip) and for the CPU (the twin at the end of this file, which evaluates the same function record by record).  The twin is what the
// kernels are tested against, what `lift --host` runs and what tests/csrc/lift_main.cpp runs under the sanitizers.  FastRemap's source is not in the reference
// tree: the function is stated here, and tests/lift_cases.py states the same rules in Python.
//
// BLOCK TABLE (host, al_lift_build).  al_chn_parse with the q side kept.  One entry per alignment line, {tSlot, tStart, size, qSlot, qStart, minus}, sorted by
// (tSlot, tStart, file index); first[s] .. first[s + 1] are slot s's entries; pmax[i] = the maximum of tStart + size over the slot's entries up to i.  q-slots:
// the distinct qNames in order of their first header, LN = qSize.  Refused, as FILE:LINE: reason: what al_chn_parse refuses, a q field that is no number, a
// qStrand other than '+' / '-', the same qName with two qSizes, a qSize of 2^31 or more, and a block of a '+' chain that ends beyond qSize (a lifted position
// then always fits the record's 32 bits).
//
// lift([s, e)) on old contig c (al_lift_iv).  i = the last entry of c's slot with tStart <= s.  The interval lifts through i iff e <= tStart_i + size_i, no
// earlier entry of the slot reaches past s (i is the slot's first, or pmax[i - 1] <= s), the slot's next entry starts at or after e, and the chain is '+'
// (an interval wholly and uniquely inside a block of a '-' chain does not lift; the block still counts for uniqueness).  Result: (qSlot_i, d = qStart_i -
// tStart_i); the new position is s + d.  A point p is [p, p + 1).  A contig the chain lacks has no entries.
//
// PER RECORD (al_lift_record).  reflen = the sum of the CIGAR operations M, D, N, =, X, 1 when that is 0; s = pos, e = pos + reflen.
//   mapped (flag & 4 clear, refID >= 0): lift([s, e)) fails -> UNLIFTED: the record leaves the BAM and becomes the BED row "chrom s e name[.1|.2] MAPQ CIGAR"
//     (old names; .1 / .2 by flag 64 / 128; CIGAR "*" when empty -- the six columns extract-reads writes).  Otherwise refID and pos are replaced and
//     bin = reg2bin(pos', pos' + reflen).
//   unmapped (flag & 4): always kept; with refID >= 0 the point (refID, pos) is lifted -- success: refID, pos replaced, bin = reg2bin(pos', pos' + 1);
//     failure: refID = pos = -1, bin = 4680.
//   mate fields of a kept record with flag & 1, flag & 8 clear and next_refID >= 0: the point (next_refID, next_pos) is lifted -- success: both replaced,
//     tlen' = tlen + (d_mate - d_own) when the two new refIDs are equal and tlen != 0, else 0; failure: next_refID = next_pos = -1, tlen = 0, flag gains
//     0x8 and loses 0x2 and 0x20.
//   Every other byte of a kept record is unchanged.  Refused: l_read_name == 0 or 32 + l_read_name + 4 * n_cigar > block_size, a name that is not
//   NUL-terminated, a refID or next_refID at or beyond the header's n_ref, and n_cigar == 2 with the kS mN sentinel (the CIGAR is in a CG tag).
//
// WALK (al_lift_walk_host, k_bam_walk).  From `start`, records follow each other by block_size; block_size < 32 or > 2^28 is malformed; the walk ends at
// the first record that is not complete within the text (`consumed` = its offset).
//
// ORDER (lift --sorted; al_lift_key, k_lift_compact / k_lift_descents / k_lift_gather_sorted, the twin's sort).  The key of a kept record, taken AFTER the lift: ~0
// (64 bits) when refID < 0, otherwise (uint64)refID << 32 | (uint32)pos -- the key of --sorted-bam (al_dev_bam.h).  Unmapped records are not dropped: a placed one
// sorts at its lifted position, one without a position sorts last.  The sorted output holds exactly the records the unsorted output holds, byte for byte, in
// non-decreasing key order; equal keys leave in input order (stable).  The rows of the unlifted records are not touched.  Per piece the kept records are compacted
// to (key, record index), the descents -- positions i of the compacted list with key[i] < key[i - 1] -- are counted, and only a piece with a descent is sorted; the
// pieces, each in order, are merged on the host (al_run_store.h).  The tie rule is this project's, as for --sorted-bam: the order is defined, not pinned to a tool.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "al_dev_chainreg.h"       // al_chn_parse; AL_DHD

struct AlLiftBlock { uint32_t tSlot, tStart, size, qSlot, qStart, minus; };
struct AlLiftTab { const AlLiftBlock *blk; const uint32_t *pmax, *first; const int32_t *ref_slot; uint32_t n_slot, n_ref; };   // ref_slot[old refID]: the chain's slot or -1
struct alignas(8) AlLiftDesc { uint32_t name_len, n_cig, mapq_flag; int32_t ref, s, pad; int64_t e; };   // in front of an unlifted record's name and CIGAR words in the arena (mapq_flag: MAPQ | flag << 8)
struct AlLiftOut { uint32_t verdict, keep_len, arena_len; };

enum { AL_LIFT_KEPT = 0, AL_LIFT_UNLIFTED = 1, AL_LIFT_UNMAPPED = 2, AL_LIFT_BAD_FIT = 3, AL_LIFT_BAD_NUL = 4, AL_LIFT_BAD_REF = 5, AL_LIFT_CG = 6, AL_LIFT_BAD_SIZE = 7, AL_LIFT_BAD_CUT = 8 };
#define AL_LIFT_MAX_BS (1 << 28)

AL_DHD uint32_t al_lift_u16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
AL_DHD uint32_t al_lift_u32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
AL_DHD void al_lift_p16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
AL_DHD void al_lift_p32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
// reg2bin of the SAM specification (section 5.3), the low 16 bits as the record holds them
AL_DHD uint32_t al_lift_reg2bin(int64_t beg, int64_t end)
{
	--end;
	if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14)) & 0xffffu;
	if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17)) & 0xffffu;
	if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20)) & 0xffffu;
	if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23)) & 0xffffu;
	if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26)) & 0xffffu;
	return 0;
}
AL_DHD bool al_lift_iv(const AlLiftTab &T, int32_t ref, int64_t s, int64_t e, int32_t *q, int64_t *d)
{
	if (ref < 0 || (uint32_t)ref >= T.n_ref) return false;
	const int32_t slot = T.ref_slot[ref];
	if (slot < 0) return false;
	const uint32_t b0 = T.first[slot], b1 = T.first[slot + 1];
	uint32_t lo = b0, hi = b1;
	while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if ((int64_t)T.blk[mid].tStart <= s) lo = mid + 1; else hi = mid; }
	if (lo == b0) return false;
	const uint32_t i = lo - 1;
	const AlLiftBlock B = T.blk[i];
	if (e > (int64_t)B.tStart + (int64_t)B.size) return false;
	if (i > b0 && (int64_t)T.pmax[i - 1] > s) return false;
	if (i + 1 < b1 && (int64_t)T.blk[i + 1].tStart < e) return false;
	if (B.minus) return false;
	*q = (int32_t)B.qSlot; *d = (int64_t)B.qStart - (int64_t)B.tStart;
	return true;
}
// the sort key of a kept record at r (its block_size field), after al_lift_record has patched it
AL_DHD uint64_t al_lift_key(const uint8_t *r) { const uint32_t ref = al_lift_u32(r + 4); return (int32_t)ref < 0 ? ~0ull : (uint64_t)ref << 32 | al_lift_u32(r + 8); }
// the reference bases the n_cig CIGAR words at c cover (c is not aligned)
AL_DHD int64_t al_lift_reflen(const uint8_t *c, uint32_t n_cig)
{
	int64_t rl = 0;
	for (uint32_t i = 0; i < n_cig; ++i) { const uint32_t w = al_lift_u32(c + 4 * i), op = w & 15; if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rl += w >> 4; }
	return rl ? rl : 1;
}
// the bytes an unlifted record takes in the arena: descriptor, name (without its NUL), CIGAR words, padded to 8
AL_DHD uint32_t al_lift_arena_len(uint32_t l_rn, uint32_t n_cig) { return (uint32_t)sizeof(AlLiftDesc) + ((l_rn - 1 + 4 * n_cig + 7u) & ~7u); }
// One record at r (its block_size field; the walk has seen that 4 + block_size bytes are there and block_size >= 32).  A kept record is patched in place.
AL_DHD AlLiftOut al_lift_record(const AlLiftTab &T, uint8_t *r)
{
	const uint32_t bs = al_lift_u32(r);
	uint8_t *b = r + 4;
	const uint32_t l_rn = b[8], n_cig = al_lift_u16(b + 12);
	uint32_t flag = al_lift_u16(b + 14);
	if (l_rn < 1 || 32 + l_rn + 4 * n_cig > bs) return AlLiftOut{AL_LIFT_BAD_FIT, 0, 0};
	if (b[32 + l_rn - 1] != 0) return AlLiftOut{AL_LIFT_BAD_NUL, 0, 0};
	const int32_t ref = (int32_t)al_lift_u32(b), pos = (int32_t)al_lift_u32(b + 4), nref = (int32_t)al_lift_u32(b + 20), npos = (int32_t)al_lift_u32(b + 24);
	if ((ref >= 0 && (uint32_t)ref >= T.n_ref) || (nref >= 0 && (uint32_t)nref >= T.n_ref)) return AlLiftOut{AL_LIFT_BAD_REF, 0, 0};
	const uint8_t *cg = b + 32 + l_rn;
	if (n_cig == 2 && (cg[0] & 15) == 4 && (cg[4] & 15) == 3) return AlLiftOut{AL_LIFT_CG, 0, 0};
	int32_t q_own = -1; int64_t d_own = 0; uint32_t verdict;
	if (!(flag & 4) && ref >= 0) {
		const int64_t rl = al_lift_reflen(cg, n_cig);
		if (!al_lift_iv(T, ref, pos, (int64_t)pos + rl, &q_own, &d_own)) return AlLiftOut{AL_LIFT_UNLIFTED, 0, al_lift_arena_len(l_rn, n_cig)};
		const int64_t np = (int64_t)pos + d_own;
		al_lift_p32(b, (uint32_t)q_own); al_lift_p32(b + 4, (uint32_t)np); al_lift_p16(b + 10, al_lift_reg2bin(np, np + rl));
		verdict = AL_LIFT_KEPT;
	} else {
		verdict = AL_LIFT_UNMAPPED;
		if ((flag & 4) && ref >= 0) {
			if (al_lift_iv(T, ref, pos, (int64_t)pos + 1, &q_own, &d_own)) {
				const int64_t np = (int64_t)pos + d_own;
				al_lift_p32(b, (uint32_t)q_own); al_lift_p32(b + 4, (uint32_t)np); al_lift_p16(b + 10, al_lift_reg2bin(np, np + 1));
			} else { q_own = -1; al_lift_p32(b, 0xffffffffu); al_lift_p32(b + 4, 0xffffffffu); al_lift_p16(b + 10, 4680); }
		}
	}
	if ((flag & 1) && !(flag & 8) && nref >= 0) {
		int32_t q_m; int64_t d_m;
		if (al_lift_iv(T, nref, npos, (int64_t)npos + 1, &q_m, &d_m)) {
			const int32_t tlen = (int32_t)al_lift_u32(b + 28);
			al_lift_p32(b + 20, (uint32_t)q_m); al_lift_p32(b + 24, (uint32_t)((int64_t)npos + d_m));
			al_lift_p32(b + 28, q_m == q_own && tlen != 0 ? (uint32_t)((int64_t)tlen + (d_m - d_own)) : 0u);
		} else {
			al_lift_p32(b + 20, 0xffffffffu); al_lift_p32(b + 24, 0xffffffffu); al_lift_p32(b + 28, 0);
			flag = (flag | 0x8u) & ~0x22u; al_lift_p16(b + 14, flag);
		}
	}
	return AlLiftOut{verdict, 4 + bs, 0};
}
// what an unlifted record (at r, untouched) leaves in the arena at a: lane `l` of `nl` copies its share of the bytes, lane 0 writes the descriptor
AL_DHD void al_lift_arena_put(const uint8_t *r, uint8_t *a, uint32_t l, uint32_t nl)
{
	const uint8_t *b = r + 4;
	const uint32_t l_rn = b[8], n_cig = al_lift_u16(b + 12), n = l_rn - 1 + 4 * n_cig, pad = (n + 7u) & ~7u;
	if (l == 0) {
		const int32_t pos = (int32_t)al_lift_u32(b + 4);
		AlLiftDesc d; d.name_len = l_rn - 1; d.n_cig = n_cig; d.mapq_flag = (uint32_t)b[9] | al_lift_u16(b + 14) << 8; d.ref = (int32_t)al_lift_u32(b); d.s = pos; d.pad = 0;
		d.e = (int64_t)pos + al_lift_reflen(b + 32 + l_rn, n_cig);
		*(AlLiftDesc *)a = d;                                               // (arena shares are multiples of 8 bytes)
	}
	uint8_t *o = a + sizeof(AlLiftDesc);
	for (uint32_t j = l; j < pad; j += nl) o[j] = j < l_rn - 1 ? b[32 + j] : j < n ? b[32 + j + 1] : (uint8_t)0;
}

static inline const char *al_lift_strerror(uint32_t code)
{
	switch (code) {
	case AL_LIFT_BAD_FIT: return "the name and the CIGAR do not fit block_size";
	case AL_LIFT_BAD_NUL: return "the name is not NUL-terminated";
	case AL_LIFT_BAD_REF: return "a refID beyond the header's list";
	case AL_LIFT_BAD_SIZE: return "block_size below 32 or above 2^28";
	case AL_LIFT_BAD_CUT: return "a record cut by the end of the file";
	default: return "?";
	}
}

// ---- the block table's builder (host) ------------------------------------------------------------------------------------------------------------------------
struct AlLiftChain {
	std::vector<std::string> tname; std::vector<uint32_t> tsize;            // the chain's slots
	std::vector<std::string> qname; std::vector<uint32_t> qsize;            // q-slots: the new reference list
	std::vector<AlLiftBlock> blk; std::vector<uint32_t> pmax, first;
	std::vector<int32_t> ref_slot;                                          // al_lift_bind
	std::unordered_map<std::string, uint32_t> t_by_name;
	AlLiftTab tab() const { return AlLiftTab{blk.data(), pmax.data(), first.data(), ref_slot.data(), (uint32_t)tname.size(), (uint32_t)ref_slot.size()}; }
};
// 0, or -1 with err = "FILE:LINE: reason"
static inline int al_lift_build(const char *fn, AlLiftChain &C, std::string &err)
{
	AlChnTab t; t.keep_q = true;
	if (al_chn_parse(fn, t, err)) return -1;
	auto fail = [&](unsigned long long ln, const std::string &why) { err = std::string(fn) + ":" + std::to_string(ln) + ": " + why; return -1; };
	C = AlLiftChain(); C.tname = t.name; C.tsize = t.L; C.t_by_name = t.by_name;
	std::unordered_map<std::string, uint32_t> q_by_name; std::vector<unsigned long long> q_line; std::vector<uint32_t> c_q(t.c_slot.size());
	for (size_t c = 0; c < t.c_slot.size(); ++c) {
		if (t.c_qsize[c] >= (1ull << 31)) return fail(t.c_line[c], "qSize is 2^31 or more");
		auto it = q_by_name.find(t.c_qname[c]);
		if (it == q_by_name.end()) { c_q[c] = (uint32_t)C.qname.size(); q_by_name[t.c_qname[c]] = c_q[c]; C.qname.push_back(t.c_qname[c]); C.qsize.push_back((uint32_t)t.c_qsize[c]); q_line.push_back(t.c_line[c]); }
		else {
			c_q[c] = it->second;
			if (C.qsize[c_q[c]] != t.c_qsize[c]) return fail(t.c_line[c], "qName '" + t.c_qname[c] + "' has qSize " + std::to_string(t.c_qsize[c]) + " here and " + std::to_string(C.qsize[c_q[c]]) + " at line " + std::to_string(q_line[c_q[c]]));
		}
	}
	C.blk.reserve(t.line.size());
	uint64_t tp = 0, qp = 0;
	for (size_t i = 0; i < t.line.size(); ++i) {
		const AlChnLine &l = t.line[i]; const uint32_t c = l.chain;
		if (i == 0 || t.line[i - 1].chain != c) { tp = t.c_tstart[c]; qp = t.c_qstart[c]; }
		if (!t.c_minus[c] && qp + l.size > t.c_qsize[c]) return fail(t.c_line[c], "a block of this chain ends beyond qSize");
		C.blk.push_back(AlLiftBlock{t.c_slot[c], (uint32_t)tp, l.size, c_q[c], t.c_minus[c] ? 0u : (uint32_t)qp, t.c_minus[c] ? 1u : 0u});
		tp += (uint64_t)l.size + l.dt; qp += (uint64_t)l.size + t.dq[i];
	}
	std::stable_sort(C.blk.begin(), C.blk.end(), [](const AlLiftBlock &a, const AlLiftBlock &b) { return a.tSlot != b.tSlot ? a.tSlot < b.tSlot : a.tStart < b.tStart; });
	C.pmax.resize(C.blk.size() + 1); C.first.assign(C.tname.size() + 1, 0);
	for (const AlLiftBlock &b : C.blk) ++C.first[b.tSlot + 1];
	for (size_t s = 0; s < C.tname.size(); ++s) C.first[s + 1] += C.first[s];
	for (size_t i = 0; i < C.blk.size(); ++i) { const uint32_t e = C.blk[i].tStart + C.blk[i].size; C.pmax[i] = (i && C.blk[i - 1].tSlot == C.blk[i].tSlot && C.pmax[i - 1] > e) ? C.pmax[i - 1] : e; }
	return 0;
}

// ---- the BAM header (host) -------------------------------------------------------------------------------------------------------------------------------------
struct AlLiftHeader { std::string text; std::vector<std::string> name; std::vector<uint32_t> len; };
// The header at h[0, n): 0 and *used = its bytes; 1: more bytes are needed; -1: malformed (err)
static inline int al_lift_header_parse(const uint8_t *h, size_t n, AlLiftHeader &H, size_t *used, std::string &err)
{
	if (n < 12) return 1;
	if (memcmp(h, "BAM\1", 4) != 0) { err = "not a BAM file (no BAM\\1 magic)"; return -1; }
	const uint32_t l_text = al_lift_u32(h + 4);
	if (l_text > (1u << 30)) { err = "the header's l_text is negative or above 2^30"; return -1; }
	if (n < 12 + (size_t)l_text) return 1;
	const uint32_t n_ref = al_lift_u32(h + 8 + l_text);
	if (n_ref > (1u << 24)) { err = "the header's n_ref is negative or above 2^24"; return -1; }
	size_t p = 12 + (size_t)l_text;
	H.text.assign((const char *)h + 8, l_text); H.name.clear(); H.len.clear();
	for (uint32_t i = 0; i < n_ref; ++i) {
		if (n < p + 4) return 1;
		const uint32_t l = al_lift_u32(h + p);
		if (l < 1 || l > (1u << 20)) { err = "a reference name's length is below 1 or above 2^20"; return -1; }
		if (n < p + 8 + (size_t)l) return 1;
		if (h[p + 4 + l - 1] != 0) { err = "a reference name is not NUL-terminated"; return -1; }
		H.name.push_back((const char *)h + p + 4); H.len.push_back(al_lift_u32(h + p + 4 + l));
		p += 8 + (size_t)l;
	}
	*used = p;
	return 0;
}
// old refID -> the chain's slot; a name in both with another length is the wrong reference
static inline int al_lift_bind(AlLiftChain &C, const AlLiftHeader &H, std::string &err)
{
	C.ref_slot.assign(H.name.size(), -1);
	for (size_t i = 0; i < H.name.size(); ++i) {
		auto it = C.t_by_name.find(H.name[i]);
		if (it == C.t_by_name.end()) continue;
		if (C.tsize[it->second] != H.len[i]) { err = "contig '" + H.name[i] + "' has length " + std::to_string(H.len[i]) + " in the BAM and tSize " + std::to_string(C.tsize[it->second]) + " in the chain file: wrong reference"; return -1; }
		C.ref_slot[i] = (int32_t)it->second;
	}
	if (C.ref_slot.empty()) C.ref_slot.reserve(1);
	return 0;
}
// an @HD line with its SO: value set: unsorted, or (sorted) coordinate, added when the line names no order
static inline std::string al_lift_hd_line(const std::string &l, bool sorted)
{
	std::string m; size_t p = 0;
	while (p <= l.size()) { size_t q = l.find('\t', p); if (q == std::string::npos) q = l.size(); std::string f = l.substr(p, q - p); if (f.compare(0, 3, "SO:") == 0) f = sorted ? "SO:coordinate" : "SO:unsorted"; if (p) m += '\t'; m += f; p = q + 1; }
	if (sorted && m.find("\tSO:") == std::string::npos) m += "\tSO:coordinate";   // (an @HD line that names no order)
	return m;
}
// The header of the lifted BAM: @SQ lines replaced by one per q-slot where the first old @SQ stood (without any: after a leading @HD, else first), an SO:
// value of @HD becomes unsorted, other lines are kept; the binary reference list is the q-slots.  sorted (lift --sorted): the SO: value becomes coordinate, and
// a text without an @HD line gets "@HD\tVN:1.6\tSO:coordinate" as its first line (the line al_bam_header writes for --sorted-bam), an @HD line without SO: gets one.
static inline void al_lift_header_write(const AlLiftHeader &H, const AlLiftChain &C, std::vector<uint8_t> &out, bool sorted = false)
{
	std::string text = H.text, tail;
	{ const size_t z = text.find('\0'); if (z != std::string::npos) { tail = text.substr(z); text.resize(z); } }   // (NUL padding stays behind the text)
	std::vector<std::string> lines;
	for (size_t p = 0; p < text.size(); ) { const size_t q = text.find('\n', p); if (q == std::string::npos) { lines.push_back(text.substr(p)); break; } lines.push_back(text.substr(p, q - p)); p = q + 1; }
	std::string sq;
	for (size_t i = 0; i < C.qname.size(); ++i) sq += "@SQ\tSN:" + C.qname[i] + "\tLN:" + std::to_string(C.qsize[i]) + "\n";
	auto is = [](const std::string &l, const char *tag) { return l.compare(0, 3, tag) == 0 && (l.size() == 3 || l[3] == '\t'); };
	bool any_sq = false;
	for (const std::string &l : lines) if (is(l, "@SQ")) any_sq = true;
	std::string o; bool put = false, any_hd = false;
	for (const std::string &l : lines) if (is(l, "@HD")) any_hd = true;
	if (sorted && !any_hd) o += "@HD\tVN:1.6\tSO:coordinate\n";
	if (!any_sq && (lines.empty() || !is(lines[0], "@HD"))) { o += sq; put = true; }
	for (size_t i = 0; i < lines.size(); ++i) {
		std::string l = lines[i];
		if (is(l, "@SQ")) { if (!put) { o += sq; put = true; } continue; }
		if (is(l, "@HD")) {
			l = al_lift_hd_line(l, sorted);
		}
		o += l; o += '\n';
		if (!put && !any_sq && i == 0) { o += sq; put = true; }
	}
	o += tail;
	out.clear();
	auto p32 = [&](uint32_t v) { uint8_t b[4]; al_lift_p32(b, v); out.insert(out.end(), b, b + 4); };
	out.insert(out.end(), {'B', 'A', 'M', 1}); p32((uint32_t)o.size()); out.insert(out.end(), o.begin(), o.end()); p32((uint32_t)C.qname.size());
	for (size_t i = 0; i < C.qname.size(); ++i) { p32((uint32_t)C.qname[i].size() + 1); out.insert(out.end(), C.qname[i].begin(), C.qname[i].end()); out.push_back(0); p32(C.qsize[i]); }
}
// the BED rows of the n_desc unlifted records of an arena
static inline void al_lift_rows(const uint8_t *arena, size_t arena_n, const AlLiftHeader &H, std::string &out)
{
	for (size_t p = 0; p + sizeof(AlLiftDesc) <= arena_n; ) {
		AlLiftDesc d; memcpy(&d, arena + p, sizeof(d));
		const uint8_t *nm = arena + p + sizeof(d), *cg = nm + d.name_len;
		const uint32_t flag = d.mapq_flag >> 8;
		out += H.name[(size_t)d.ref]; out += '\t'; out += std::to_string(d.s); out += '\t'; out += std::to_string(d.e); out += '\t';
		out.append((const char *)nm, d.name_len); if (flag & 64) out += ".1"; else if (flag & 128) out += ".2";
		out += '\t'; out += std::to_string(d.mapq_flag & 0xff); out += '\t';
		if (d.n_cig == 0) out += '*';
		for (uint32_t i = 0; i < d.n_cig; ++i) { const uint32_t w = al_lift_u32(cg + 4 * i); out += std::to_string(w >> 4); out += "MIDNSHP=X???????"[w & 15]; }
		out += '\n';
		p += al_lift_arena_len(d.name_len + 1, d.n_cig);
	}
}

// ---- the host twin -------------------------------------------------------------------------------------------------------------------------------------------
// What k_bam_walk computes: rec_off of the complete records of t[start, n), *consumed, *bad (1: the record at *consumed has a block_size out of range)
static inline void al_lift_walk_host(const uint8_t *t, uint64_t n, uint64_t start, std::vector<uint32_t> &rec_off, uint64_t *consumed, uint32_t *bad)
{
	rec_off.clear(); *bad = 0;
	uint64_t p = start;
	while (p + 4 <= n) {
		const uint32_t bs = al_lift_u32(t + p);
		if (bs < 32 || bs > AL_LIFT_MAX_BS) { *bad = 1; break; }
		if (p + 4 + bs > n) break;
		rec_off.push_back((uint32_t)p); p += 4 + (uint64_t)bs;
	}
	*consumed = p;
}

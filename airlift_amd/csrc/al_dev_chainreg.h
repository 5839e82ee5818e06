// al_dev_chainreg.h -- the chain file's region logic (`chain-beds`, `tokens --chain`) as ONE function of the parsed chain file, written once for both sides:
// the pieces below are compiled for the device (k_chn_expand, the fold, k_chn_invert: al_chainreg.hip) and for the CPU (the twin in this file, which evaluates
// the same function serially).  The twin is what the kernels are tested against, what `chain-beds --host` runs and what tests/csrc/chainreg_main.cpp runs
// under the sanitizers.  It replaces 2_get_updated_regions_bed.py (the gaps BED), get_constant_regions.py and get_retired_regions.py of the reference.
//
// PARSING (host, one pass, al_chn_parse).  '#' as first byte: a comment; blank lines are skipped; a line whose first field is "chain": a header
// "chain score tName tSize tStrand tStart tEnd qName qSize qStrand qStart qEnd id"; every other line is an alignment line "size dt dq" or "size" (the last
// line of its chain).  The distinct tNames in order of their first header are the SLOTS s, L[s] the tSize of the slot's first header.  Refused, as
// FILE:LINE: reason: a data line before the first header, a field count other than 1 or 3, a non-numeric field, size == 0, a data line after a chain's
// 1-field line, tSize >= 2^31, a tStrand other than '+', a block or gap that ends beyond L[slot].  The last rule is what lets every interval below fit 32
// bits and keeps every padded interval the right way round (start <= end).
//
// THE FUNCTION.  Alignment lines i = 0..N-1 in file order, {chain, size, dt (0 on a 1-field line), three}:
//  1. T[i] = tStart[chain[i]] + sum of size[j] + dt[j] over the earlier lines j of the same chain: a segmented exclusive scan (al_chn_sum_op).
//  2. Block B[i] = [T, T + size - 1] (inclusive) for every line; gap G[i] = [T + size, T + size + dt - 1] for every 3-field line (dt = 0: the empty
//     [g, g - 1], kept: once padded it marks the surroundings of an insertion).
//  3. pad([a, b], p, L) = [a >= p ? a - p : 0, b + p <= L - 1 ? b + p : L - 1]                                         (al_chn_pad)
//  4. merge(strict): order (slot, start, input index); within a slot an element joins the current region iff start < region.end (strict) or
//     start <= region.end; the region's end becomes the maximum.                                                         (AlChnFold, al_dev_fold.h)
//  5. Gaps rows = merge(strict) over pad(G[i], R + E, L[slot]), slot by slot.
//  6. Constant rows = B[i], unpadded, unmerged, ordered (slot, input index).
//  7. Retired rows, given merged regions M (rows "contig start end", the numbers as written, inclusive): the slots of this step are M's contigs in order
//     of first appearance, then the chain's tNames not among them in chain order; U = pad(M u B, R, L), M's rows before the blocks; r_0..r_{k-1} per
//     slot = merge(not strict); holes [0, r_0.start - 1] if r_0.start > 0 and [r_{j-1}.end + 1, r_j.start - 1] where not empty; the tail
//     [r_{k-1}.end + 1, L - 1] only when the slot already has a hole and r_{k-1}.end < L - 1 (the script's rule, kept as it is: a contig covered from its
//     first base and bare behind gets no row).
//
// FORM OF THE MERGE.  The device compares an element's start with the running maximum of `end` over the slot's PREFIX in sorted order (one segmented scan,
// al_fold_scan_op of al_dev_fold.h), the scripts and the twin with the maximum over the current REGION.  They are the same number: every element of an earlier region
// of the slot ends at or before (strict) / before (not strict) the start of the head of the next region, that start is <= every later start of the slot
// (sorted), and every start is <= its own end (no inverted interval: the parser's last rule, p >= 1 for the empty gaps, and M's rows are refused unless
// start <= end and start < L).  So the earlier regions' maxima never exceed an end of the current region, and the prefix maximum is the region's.
#pragma once
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <vector>
#include <unordered_map>
#include "al_dev_regions.h"       // AlRegIv; al_dev_fold.h

struct alignas(16) AlChnLine { uint32_t chain, size, dt, three; };
struct alignas(16) AlChnIv { uint32_t slot, start, end, idx; };
#define AL_CHN_NONE 0xffffffffu      // the slot of an element that is none (a 1-field line has no gap; a region without a hole)

AL_DHD bool al_chn_less(const AlChnIv &a, const AlChnIv &b)
{
	if (a.slot != b.slot) return a.slot < b.slot;
	if (a.start != b.start) return a.start < b.start;
	return a.idx < b.idx;
}
AL_DHD bool al_chn_less_idx(const AlChnIv &a, const AlChnIv &b) { return a.slot != b.slot ? a.slot < b.slot : a.idx < b.idx; }   // (the constant rows)
// the scan of T: bit 32 = a chain starts at (or inside) what the element covers, low word = the sum of size + dt since then (below 2^31: it ends within L)
AL_DHD uint64_t al_chn_sum_elem(bool chain_start, uint32_t v) { return (chain_start ? 1ull << 32 : 0ull) | v; }
AL_DHD uint64_t al_chn_sum_op(uint64_t a, uint64_t b)
{
	const uint32_t va = (uint32_t)a, vb = (uint32_t)b;
	return ((a | b) & (1ull << 32)) | ((b >> 32 & 1) ? vb : (uint32_t)(va + vb));
}
AL_DHD void al_chn_pad(uint32_t a, uint32_t b, uint32_t p, uint32_t L, uint32_t *o_a, uint32_t *o_b)
{
	*o_a = a >= p ? a - p : 0;
	*o_b = (uint64_t)b + p + 1 <= (uint64_t)L ? b + p : L - 1;
}
// line i, T = the first target base of its block: the padded gap (slot AL_CHN_NONE on a 1-field line) and the block padded by p_blk (0: as it is)
AL_DHD AlChnIv al_chn_gap(const AlChnLine &l, uint32_t T, uint32_t slot, uint32_t p, uint32_t L, uint32_t idx)
{
	AlChnIv v{AL_CHN_NONE, 0, 0, idx};
	if (!l.three) return v;
	const uint32_t g = T + l.size;                                        // g >= 1 (size > 0), g + dt <= L
	v.slot = slot; al_chn_pad(g, g + l.dt - 1, p, L, &v.start, &v.end);
	return v;
}
AL_DHD AlChnIv al_chn_block(const AlChnLine &l, uint32_t T, uint32_t slot, uint32_t p, uint32_t L, uint32_t idx)
{
	AlChnIv v{slot, T, T + l.size - 1, idx};
	if (p) al_chn_pad(v.start, v.end, p, L, &v.start, &v.end);
	return v;
}
// the fold of al_dev_fold.h: a segment per slot; a region's idx is its number
struct AlChnFold {
	typedef AlChnIv Elem;
	AL_DHD_M bool less(const AlChnIv &a, const AlChnIv &b) { return al_chn_less(a, b); }
	AL_DHD_M bool same_seg(const AlChnIv &a, const AlChnIv &b) { return a.slot == b.slot; }
	AL_DHD_M void head(AlChnIv &r, const AlChnIv &h, uint32_t k) { r.slot = h.slot; r.start = h.start; r.idx = k; }
};
// region j of the sorted regions r[0, k): its leading hole (slot AL_CHN_NONE: none)
AL_DHD AlChnIv al_chn_hole(const AlChnIv *r, uint64_t j)
{
	AlChnIv h{AL_CHN_NONE, 0, 0, 0};
	const bool first = j == 0 || r[j - 1].slot != r[j].slot;
	const uint32_t lo = first ? 0 : r[j - 1].end + 1;
	if (r[j].start > lo) h = AlChnIv{r[j].slot, lo, r[j].start - 1, 0};   // (first: start > 0; otherwise start - 1 >= end' + 1)
	return h;
}
// ... and its tail, when it is the last of its slot, the slot has `holes` holes and the region ends before the contig
AL_DHD AlChnIv al_chn_tail(const AlChnIv *r, uint64_t k, uint64_t j, uint32_t holes, uint32_t L)
{
	AlChnIv h{AL_CHN_NONE, 0, 0, 0};
	const bool last = j + 1 == k || r[j + 1].slot != r[j].slot;
	if (last && holes && (uint64_t)r[j].end + 1 < (uint64_t)L) h = AlChnIv{r[j].slot, r[j].end + 1, L - 1, 0};
	return h;
}

// what the function is evaluated on: the line table, and for the retired step the merged regions and the slots of that step
struct AlChnIn {
	uint64_t n = 0; const AlChnLine *line = nullptr;
	uint32_t n_chain = 0; const uint32_t *c_slot = nullptr, *c_tstart = nullptr;
	uint32_t n_slot = 0; const uint32_t *L = nullptr;
	// the retired step: M's rows {slot of this step, start, end} on the host, or (tokens) where the run's merged regions lie on the device, as
	// AlRegIv {0, rank, start, end} with rank_rslot[rank] the slot of this step; rslot_of[s] is the slot of chain slot s, RL[] the lengths
	uint64_t n_m = 0; const AlChnIv *M = nullptr; const AlRegIv *dev_M = nullptr; const uint32_t *rank_rslot = nullptr; uint32_t n_rank = 0;
	uint32_t n_rslot = 0; const uint32_t *rslot_of = nullptr, *RL = nullptr;
};

// what the parser guarantees of a table, checked where a table comes from elsewhere (the test taps): null, or what is wrong
static inline const char *al_chn_in_bad(const AlChnIn &in, bool ret)
{
	if (in.n >= 0x7ffffff0ull || in.n + in.n_m >= 0x7ffffff0ull) return "more lines than a run takes";
	for (uint32_t c = 0; c < in.n_chain; ++c) if (in.c_slot[c] >= in.n_slot || in.c_tstart[c] > in.L[in.c_slot[c]]) return "a chain's slot or tStart lies outside the tables";
	for (uint32_t s = 0; s < in.n_slot; ++s) if (in.L[s] >= (1u << 31) || (ret && (in.rslot_of[s] >= in.n_rslot || in.RL[in.rslot_of[s]] != in.L[s]))) return "a slot's length or its slot of the retired step is wrong";
	uint64_t pos = 0;
	for (uint64_t i = 0; i < in.n; ++i) {
		const AlChnLine &l = in.line[i];
		if (l.chain >= in.n_chain || (i && l.chain < in.line[i - 1].chain)) return "a line's chain lies outside the table or before the line's predecessor's";
		if (i == 0 || l.chain != in.line[i - 1].chain) pos = in.c_tstart[l.chain];
		if (l.size == 0 || (!l.three && l.dt)) return "a line has size 0, or a dt without three fields";
		pos += (uint64_t)l.size + l.dt;
		if (pos > in.L[in.c_slot[l.chain]]) return "a block or gap ends beyond tSize";
	}
	if (ret) for (uint64_t i = 0; i < in.n_m; ++i) if (in.M[i].slot >= in.n_rslot || in.M[i].start > in.M[i].end || in.M[i].start >= in.RL[in.M[i].slot]) return "a merged row lies outside its tables or its contig";
	return nullptr;
}

// ---- the host twin -------------------------------------------------------------------------------------------------------------------------------------------
static inline void al_chn_T_host(const AlChnIn &in, std::vector<uint32_t> &T)
{
	T.resize(in.n);
	uint64_t acc = 0;
	for (uint64_t i = 0; i < in.n; ++i) {
		const AlChnLine &l = in.line[i];
		acc = al_chn_sum_op(acc, al_chn_sum_elem(i == 0 || in.line[i - 1].chain != l.chain, l.size + l.dt));
		T[i] = in.c_tstart[l.chain] + (uint32_t)acc - (l.size + l.dt);
	}
}
static inline void al_chn_gaps_host(const AlChnIn &in, const uint32_t *T, uint32_t p, std::vector<AlChnIv> &rows)
{
	rows.clear();
	for (uint64_t i = 0; i < in.n; ++i) {
		const uint32_t s = in.c_slot[in.line[i].chain];
		const AlChnIv g = al_chn_gap(in.line[i], T[i], s, p, in.L[s], (uint32_t)i);
		if (g.slot != AL_CHN_NONE) rows.push_back(g);
	}
	al_fold_host<AlChnFold>(rows, true);
}
static inline void al_chn_constant_host(const AlChnIn &in, const uint32_t *T, std::vector<AlChnIv> &rows)
{
	rows.clear();
	for (uint64_t i = 0; i < in.n; ++i) { const uint32_t s = in.c_slot[in.line[i].chain]; rows.push_back(al_chn_block(in.line[i], T[i], s, 0, in.L[s], (uint32_t)i)); }
	std::stable_sort(rows.begin(), rows.end(), [](const AlChnIv &a, const AlChnIv &b) { return al_chn_less_idx(a, b); });
}
static inline void al_chn_retired_host(const AlChnIn &in, const uint32_t *T, uint32_t p, std::vector<AlChnIv> &rows)
{
	std::vector<AlChnIv> u; u.reserve(in.n_m + in.n);
	for (uint64_t i = 0; i < in.n_m; ++i) { AlChnIv v = in.M[i]; v.idx = (uint32_t)i; al_chn_pad(v.start, v.end, p, in.RL[v.slot], &v.start, &v.end); u.push_back(v); }
	for (uint64_t i = 0; i < in.n; ++i) {
		const uint32_t s = in.rslot_of[in.c_slot[in.line[i].chain]];
		AlChnIv v = al_chn_block(in.line[i], T[i], s, 0, in.RL[s], (uint32_t)(in.n_m + i));
		al_chn_pad(v.start, v.end, p, in.RL[s], &v.start, &v.end);        // (p may be 0: the pad of nothing)
		u.push_back(v);
	}
	al_fold_host<AlChnFold>(u, false);
	rows.clear();
	std::vector<uint32_t> holes(in.n_rslot, 0);
	for (size_t j = 0; j < u.size(); ++j) {
		const AlChnIv h = al_chn_hole(u.data(), j);
		if (h.slot != AL_CHN_NONE) { rows.push_back(h); ++holes[h.slot]; }
		const AlChnIv t = al_chn_tail(u.data(), u.size(), j, holes[u[j].slot], in.RL[u[j].slot]);   // (the last region of a slot: its holes are all counted)
		if (t.slot != AL_CHN_NONE) rows.push_back(t);
	}
}

// ---- the chain file ------------------------------------------------------------------------------------------------------------------------------------------
struct AlChnTab {
	std::vector<std::string> name; std::vector<uint32_t> L; std::vector<unsigned long long> first_line;   // slots (and the line of their first header)
	std::vector<uint32_t> c_slot, c_tstart;                              // chains
	std::vector<AlChnLine> line;
	uint64_t n_three = 0;
	std::unordered_map<std::string, uint32_t> by_name;
	// the q side, kept only when keep_q is set before al_chn_parse (lift, al_dev_lift.h): per chain qName, qSize, qStart, qStrand == '-' and the line of its
	// header; per alignment line dq (0 on a 1-field line)
	bool keep_q = false;
	std::vector<std::string> c_qname; std::vector<uint64_t> c_qsize, c_qstart; std::vector<uint8_t> c_minus; std::vector<unsigned long long> c_line; std::vector<uint32_t> dq;
	AlChnIn in() const
	{
		AlChnIn x; x.n = line.size(); x.line = line.data(); x.n_chain = (uint32_t)c_slot.size(); x.c_slot = c_slot.data(); x.c_tstart = c_tstart.data();
		x.n_slot = (uint32_t)L.size(); x.L = L.data();
		return x;
	}
};
static inline bool al_chn_num(const char *s, size_t n, uint64_t *v)
{
	if (n == 0) return false;
	uint64_t x = 0;
	for (size_t i = 0; i < n; ++i) { if (s[i] < '0' || s[i] > '9') return false; x = x * 10 + (uint64_t)(s[i] - '0'); if (x > (1ull << 40)) x = 1ull << 40; }
	*v = x;
	return true;
}
// the fields of a line (split at blanks, as str.split() does)
static inline void al_chn_fields(const char *l, size_t n, std::vector<std::pair<size_t, size_t>> &f, size_t most)
{
	f.clear();
	size_t i = 0;
	auto blank = [](char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n' || c == '\v' || c == '\f'; };
	while (i < n && f.size() < most) {
		while (i < n && blank(l[i])) ++i;
		if (i >= n) break;
		const size_t a = i;
		while (i < n && !blank(l[i])) ++i;
		f.push_back({a, i - a});
	}
}
struct AlChnLineReader {                                                  // whole lines of a file, however long
	FILE *fp = nullptr; char *buf = nullptr; size_t cap = 0; unsigned long long n_line = 0;
	bool open(const char *fn) { fp = fopen(fn, "rb"); return fp != nullptr; }
	bool next(const char **l, size_t *n) { const ssize_t r = getline(&buf, &cap, fp); if (r < 0) return false; ++n_line; *l = buf; *n = (size_t)r; return true; }
	~AlChnLineReader() { if (fp) fclose(fp); free(buf); }
};
// 0, or -1 with err = "FILE:LINE: reason" (or "FILE: reason")
static inline int al_chn_parse(const char *fn, AlChnTab &t, std::string &err)
{
	AlChnLineReader rd;
	if (!rd.open(fn)) { err = std::string(fn) + ": cannot be opened"; return -1; }
	auto fail = [&](const char *why) { err = std::string(fn) + ":" + std::to_string(rd.n_line) + ": " + why; return -1; };
	std::vector<std::pair<size_t, size_t>> f;
	const char *l; size_t n; bool have = false, closed = false; uint64_t pos = 0; uint32_t slot = 0;
	while (rd.next(&l, &n)) {
		if (n && l[0] == '#') continue;
		al_chn_fields(l, n, f, 14);
		if (f.empty()) continue;
		if (f[0].second == 5 && !memcmp(l + f[0].first, "chain", 5)) {
			if (f.size() < 13) return fail("a chain header with fewer than 13 fields");
			uint64_t tsize, tstart;
			if (!al_chn_num(l + f[3].first, f[3].second, &tsize)) return fail("tSize is not a number");
			if (!al_chn_num(l + f[5].first, f[5].second, &tstart)) return fail("tStart is not a number");
			if (tsize >= (1ull << 31)) return fail("tSize is 2^31 or more");
			if (f[4].second != 1 || l[f[4].first] != '+') return fail("tStrand is not '+'");
			const std::string nm(l + f[2].first, f[2].second);
			auto it = t.by_name.find(nm);
			if (it == t.by_name.end()) { slot = (uint32_t)t.name.size(); t.by_name[nm] = slot; t.name.push_back(nm); t.L.push_back((uint32_t)tsize); t.first_line.push_back(rd.n_line); }
			else slot = it->second;                                          // (a later header's tSize changes nothing, as in the scripts)
			if (tstart > t.L[slot]) return fail("tStart lies beyond tSize");
			if (t.c_slot.size() >= 0xfffffffeu) return fail("more chains than a run takes");
			if (t.keep_q) {
				uint64_t qsize, qstart;
				if (!al_chn_num(l + f[8].first, f[8].second, &qsize)) return fail("qSize is not a number");
				if (!al_chn_num(l + f[10].first, f[10].second, &qstart)) return fail("qStart is not a number");
				if (f[9].second != 1 || (l[f[9].first] != '+' && l[f[9].first] != '-')) return fail("qStrand is neither '+' nor '-'");
				t.c_qname.push_back(std::string(l + f[7].first, f[7].second)); t.c_qsize.push_back(qsize); t.c_qstart.push_back(qstart);
				t.c_minus.push_back(l[f[9].first] == '-'); t.c_line.push_back(rd.n_line);
			}
			t.c_slot.push_back(slot); t.c_tstart.push_back((uint32_t)tstart);
			pos = tstart; have = true; closed = false;
			continue;
		}
		if (!have) return fail("an alignment line before the first chain header");
		if (closed) return fail("a line after the chain's last (1-field) line that is no header");
		if (f.size() != 1 && f.size() != 3) return fail("an alignment line has 1 or 3 fields");
		uint64_t v[3] = {0, 0, 0};
		for (size_t j = 0; j < f.size(); ++j) if (!al_chn_num(l + f[j].first, f[j].second, &v[j])) return fail("a field is not a number");
		if (v[0] == 0) return fail("size is 0");
		if (pos + v[0] > t.L[slot]) return fail("the block ends beyond tSize");
		if (pos + v[0] + v[1] > t.L[slot]) return fail("the gap ends beyond tSize");
		if (t.line.size() >= 0x7ffffff0u) return fail("more alignment lines than a run takes");
		if (t.keep_q) { if (v[2] >= (1ull << 31)) return fail("dq is 2^31 or more"); t.dq.push_back((uint32_t)v[2]); }
		t.line.push_back(AlChnLine{(uint32_t)t.c_slot.size() - 1, (uint32_t)v[0], (uint32_t)v[1], f.size() == 3 ? 1u : 0u});
		pos += v[0] + v[1];
		if (f.size() == 3) ++t.n_three; else closed = true;
	}
	return 0;
}

// the slots of the retired step: M's contigs `m_names` (distinct, in order of first appearance), then the chain's other tNames.  len_of(name): the length
// of a contig no header names, or -1.  -1: *bad = the index of the name without a length.
struct AlChnRet { std::vector<std::string> name; std::vector<uint32_t> L, rslot_of; std::vector<AlChnIv> M; std::unordered_map<std::string, uint32_t> by_name; };
template <class F>
static inline int al_chn_ret_slots(const AlChnTab &t, const std::vector<std::string> &m_names, F len_of, AlChnRet &r, size_t *bad)
{
	r.name.clear(); r.L.clear(); r.by_name.clear(); r.rslot_of.assign(t.name.size(), 0);
	for (size_t i = 0; i < m_names.size(); ++i) {
		auto it = t.by_name.find(m_names[i]);
		int64_t len = it != t.by_name.end() ? (int64_t)t.L[it->second] : (int64_t)len_of(m_names[i]);
		if (len < 0) { *bad = i; return -1; }
		r.by_name[m_names[i]] = (uint32_t)r.name.size(); r.name.push_back(m_names[i]); r.L.push_back((uint32_t)len);
	}
	for (size_t s = 0; s < t.name.size(); ++s) {
		auto it = r.by_name.find(t.name[s]);
		if (it == r.by_name.end()) { r.by_name[t.name[s]] = (uint32_t)r.name.size(); r.rslot_of[s] = (uint32_t)r.name.size(); r.name.push_back(t.name[s]); r.L.push_back(t.L[s]); }
		else r.rslot_of[s] = it->second;
	}
	return 0;
}
static inline void al_chn_ret_in(const AlChnRet &r, AlChnIn &x)
{
	x.n_m = r.M.size(); x.M = r.M.data(); x.n_rslot = (uint32_t)r.name.size(); x.rslot_of = r.rslot_of.data(); x.RL = r.L.data();
}
// one retired-step row of M, its numbers as written (inclusive): refused unless start <= end and start < L (what keeps the padded row the right way round)
static inline const char *al_chn_m_row_bad(uint64_t start, uint64_t end, uint32_t L)
{
	if (start > end) return "the end lies before the start";
	if (start >= L) return "the start lies beyond the contig";
	return nullptr;
}
// the merged BED of `chain-beds --merged-in`: rows "contig start end" (split at blanks, further fields ignored, blank lines skipped); a contig no header
// names is refused (there is no index to take its length from)
static inline int al_chn_parse_merged(const char *fn, const AlChnTab &t, AlChnRet &r, std::string &err)
{
	AlChnLineReader rd;
	if (!rd.open(fn)) { err = std::string(fn) + ": cannot be opened"; return -1; }
	auto fail = [&](unsigned long long line, const char *why) { err = std::string(fn) + ":" + std::to_string(line) + ": " + why; return -1; };
	struct Row { uint32_t name; uint64_t start, end; unsigned long long line; };
	std::vector<Row> rows; std::vector<std::string> names; std::vector<unsigned long long> first_line; std::unordered_map<std::string, uint32_t> seen;
	std::vector<std::pair<size_t, size_t>> f; const char *l; size_t n;
	while (rd.next(&l, &n)) {
		al_chn_fields(l, n, f, 4);
		if (f.empty()) continue;
		if (f.size() < 3) return fail(rd.n_line, "fewer than three fields");
		Row w; w.line = rd.n_line;
		if (!al_chn_num(l + f[1].first, f[1].second, &w.start)) return fail(rd.n_line, "the start is not a number");
		if (!al_chn_num(l + f[2].first, f[2].second, &w.end)) return fail(rd.n_line, "the end is not a number");
		const std::string nm(l + f[0].first, f[0].second);
		auto it = seen.find(nm);
		if (it == seen.end()) { w.name = (uint32_t)names.size(); seen[nm] = w.name; names.push_back(nm); first_line.push_back(rd.n_line); } else w.name = it->second;
		rows.push_back(w);
	}
	size_t bad = 0;
	if (al_chn_ret_slots(t, names, [](const std::string &) { return -1; }, r, &bad) != 0) return fail(first_line[bad], "no chain header names this contig");
	r.M.clear();
	for (const Row &w : rows) {                                           // (slot of this step == index among the names)
		const char *why = al_chn_m_row_bad(w.start, w.end, r.L[w.name]);
		if (why) return fail(w.line, why);
		r.M.push_back(AlChnIv{w.name, (uint32_t)w.start, (uint32_t)std::min<uint64_t>(w.end, 0xfffffff0u), 0});
	}
	if (r.M.size() + t.line.size() >= 0x7ffffff0u) { err = std::string(fn) + ": more rows than a run takes"; return -1; }
	return 0;
}

// BED text of rows in their order: "name\tstart\tend\n", inclusive, as the scripts print them
static inline void al_chn_bed(std::string &o, const AlChnIv *v, size_t n, const std::vector<std::string> &name)
{
	char num[40];
	for (size_t i = 0; i < n; ++i) {
		o += name[v[i].slot];
		o.append(num, (size_t)snprintf(num, sizeof(num), "\t%u\t%u\n", v[i].start, v[i].end));
	}
}

// the whole function on the twin; p_gap < 0: no gaps rows; constant / retired may be null (retired needs in.M / RL)
static inline void al_chainreg_host(const AlChnIn &in, int R, int E, std::vector<AlChnIv> *gaps, std::vector<AlChnIv> *constant, std::vector<AlChnIv> *retired)
{
	std::vector<uint32_t> T; al_chn_T_host(in, T);
	if (gaps) al_chn_gaps_host(in, T.data(), (uint32_t)(R + E), *gaps);
	if (constant) al_chn_constant_host(in, T.data(), *constant);
	if (retired) al_chn_retired_host(in, T.data(), (uint32_t)R, *retired);
}

// ---- the device form (al_chainreg.hip) -----------------------------------------------------------------------------------------------------------------------
// Uploads the line table, runs the scan, k_chn_expand, the folds and k_chn_invert on `device` and copies only the result rows back; every device buffer is
// obtained through al_dev_malloc and released before it returns.  in.dev_M: the merged regions are read where they lie.
struct AlChnStat { double ms_kernels = 0; uint64_t bytes_h2d = 0, bytes_d2h = 0; };
int al_chainreg_device(int device, const AlChnIn &in, int R, int E, std::vector<AlChnIv> *gaps, std::vector<AlChnIv> *constant, std::vector<AlChnIv> *retired, AlChnStat *st);

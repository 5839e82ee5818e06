// al_dev_merge.h -- `merge`: 2 to 8 coordinate-sorted BAMs merged into one (run_pipeline.sh:116 and :119, samtools merge) as ONE function of the inputs' headers
// and records, written once for both sides: the pieces below are compiled for the device (k_merge_key, k_merge_descents, k_merge_bounds: al_merge.hip) and for the
// CPU (the twin in al_merge.h, which evaluates the same function).  The twin is what the kernels are tested against, what `merge --host` runs and what
// tests/csrc/merge_main.cpp runs under the sanitizers.  tests/merge_cases.py states the same rules in Python.
//
// KEY.  al_lift_key (al_dev_lift.h) as it stands, taken AFTER the refID translation below: ~0 (64 bits) when refID < 0, otherwise (uint64)refID << 32 | (uint32)pos.
//
// ORDER.  The output holds exactly the records of all inputs in non-decreasing key order, each byte for byte as read except the two translated fields.  Among
// equal keys the records of an earlier input (by argument order) come first; within one input, input order holds.  The tie rule is this project's, as for
// --sorted-bam and lift --sorted: the order is defined, not pinned to a tool.  Nothing is sorted here: an input whose keys descend anywhere -- across a piece
// boundary too -- is refused with "not in coordinate order at offset N of the inflated stream", N being the offset of the record that is smaller than the one
// before it.
//
// REFERENCE LISTS (al_merge_headers).  The output's list is input 1's; contigs of later inputs that the list lacks are appended in the order they are first met;
// contigs are matched by name.  Each input gets a table old refID -> new refID (input 1's is the identity); refID and next_refID of its records are replaced
// (al_merge_record), a negative value stays as it is, and `bin` does not depend on refID.  Refused, with the file and the contigs named: a contig whose LN differs
// between inputs; a table that is not strictly increasing (the input would no longer be in order; the two contigs that are out of order are named); and, per
// record, a refID or next_refID at or beyond the input's own n_ref (lift's message).
//
// HEADER TEXT (al_merge_headers).  Input 1's text up to its first NUL, line by line: an @HD line gets SO:coordinate by the rule of al_lift_hd_line (a text without
// @HD gets "@HD\tVN:1.6\tSO:coordinate" as its first line); every other line stays.  Then, for each later input K = 2, 3, ... in turn (its text up to its first NUL,
// empty lines skipped): first one @SQ line per contig it appended -- its own @SQ line with that SN, or "@SQ\tSN:name\tLN:len" when its text has none -- then
// every other line of it: @HD lines and the remaining @SQ lines are dropped (the list above stands for them); an @CO line is appended as it is; any other line
// is dropped when a byte-identical line is already present; a @PG line whose ID is already the ID of a @PG line present is appended with ID:x.K (its PP: is left
// alone); a @RG line whose ID is already the ID of a @RG line present is refused (the records' RG:Z would have to be rewritten); everything else is appended.
// Every line ends in a newline; what followed input 1's first NUL stays behind the text.
//
// MALFORMED RECORDS.  The walk's rules (al_dev_lift.h, WALK): block_size < 32 or > 2^28, or a file that ends inside a record, with lift's message.
//
// THE STREAMING RULE (al_merge_emit_count).  Each input holds a window: whole records of its stream with their offsets and keys, a cursor c_i, and eof_i (the
// window reaches the input's end).  L_i = the last key of a non-eof input's window, B = the minimum of the L_i, j* = the smallest input index that attains it.  A
// round emits, from each input, the records at or after its cursor with key <= B when i <= j*, with key < B when i > j* (j* may bring more records equal to B
// later, and those must still precede the equal records of later inputs), and everything left when every input is at eof.  Input j* always empties its window;
// an input whose window is empty and that is not at eof is refilled before the next round (carry of the incomplete tail, the next piece, inflate, walk, keys;
// a refill that yields no complete record doubles that input's piece), and partly consumed windows stay where they are.
//
// TAGS.  A record in a round is named by tag = input << 28 | record index in the input's window: a window holds fewer than 2^28 records, larger ones are refused.
#pragma once
#include <stdint.h>
#include <string.h>
#include <string>
#include <unordered_map>
#include <vector>
#include "al_dev_lift.h"

#define AL_MERGE_MAX_IN 8
#define AL_MERGE_THREADS 256u                                   // lanes of a k_merge_tile block
#define AL_MERGE_VT 4u                                          // consecutive outputs per lane
#define AL_MERGE_TILE (AL_MERGE_THREADS * AL_MERGE_VT)          // outputs per block (the reasoning: al_merge.hip)
#define AL_MERGE_TAG_BITS 28
#define AL_MERGE_TAG_MASK ((1u << AL_MERGE_TAG_BITS) - 1)

struct AlMergeWin { const uint64_t *key; uint32_t cur, n, eof; };   // one input's window: its keys, the cursor, the records, 1 when the window reaches the input's end
struct AlMergeWins { AlMergeWin w[AL_MERGE_MAX_IN]; uint32_t k; };
struct AlMergePtrs { const uint8_t *txt[AL_MERGE_MAX_IN]; const uint32_t *rec_off[AL_MERGE_MAX_IN]; const uint32_t *rlen[AL_MERGE_MAX_IN]; };   // what a tag's input field chooses

// One record at r (its block_size field; the walk has seen that 4 + block_size bytes are there and block_size >= 32) of an input with n_ref contigs and the
// table `map`: refID and next_refID translated in place, *key and *len (4 + block_size) set.  0, or AL_LIFT_BAD_REF (nothing is written to the record, *key = 0).
AL_DHD uint32_t al_merge_record(uint8_t *r, const int32_t *map, uint32_t n_ref, uint64_t *key, uint32_t *len)
{
	uint8_t *b = r + 4;
	const int32_t ref = (int32_t)al_lift_u32(b), nref = (int32_t)al_lift_u32(b + 20);
	*len = 4 + al_lift_u32(r);
	if ((ref >= 0 && (uint32_t)ref >= n_ref) || (nref >= 0 && (uint32_t)nref >= n_ref)) { *key = 0; return AL_LIFT_BAD_REF; }
	if (ref >= 0 && map[ref] != ref) al_lift_p32(b, (uint32_t)map[ref]);
	if (nref >= 0 && map[nref] != nref) al_lift_p32(b + 20, (uint32_t)map[nref]);
	*key = al_lift_key(r);
	return 0;
}
// The streaming rule: the records input i emits in the round the windows W stand before.  Every non-eof input has a record at or after its cursor.
AL_DHD uint32_t al_merge_emit_count(const AlMergeWins &W, uint32_t i)
{
	uint64_t B = 0; uint32_t js = 0; bool have = false;
	for (uint32_t j = 0; j < W.k; ++j) {
		if (W.w[j].eof || W.w[j].n == 0) continue;
		const uint64_t L = W.w[j].key[W.w[j].n - 1];
		if (!have || L < B) { B = L; js = j; have = true; }
	}
	const AlMergeWin &w = W.w[i];
	if (!have) return w.n - w.cur;                                  // every input is at eof: everything left
	const bool incl = i <= js;
	uint32_t lo = w.cur, hi = w.n;                                  // the first record at or after the cursor that stays
	while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; const uint64_t k = w.key[mid]; if (incl ? k <= B : k < B) lo = mid + 1; else hi = mid; }
	return lo - w.cur;
}
// The split of diagonal d of the stable merge of a[0, na) and b[0, nb): how many of the first d outputs come from a, which wins ties.
AL_DHD uint32_t al_merge_path(const uint64_t *a, uint32_t na, const uint64_t *b, uint32_t nb, uint32_t d)
{
	uint32_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
	while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (a[mid] <= b[d - 1 - mid]) lo = mid + 1; else hi = mid; }
	return lo;
}

// ---- the headers (host) ------------------------------------------------------------------------------------------------------------------------------------------
struct AlMergeHeaders { std::vector<uint8_t> out; std::vector<std::string> name; std::vector<uint32_t> len; std::vector<std::vector<int32_t>> map; };
static inline bool al_merge_is(const std::string &l, const char *tag) { return l.compare(0, 3, tag) == 0 && (l.size() == 3 || l[3] == '\t'); }
// the value of the line's first field that begins with `pre` ("ID:", "SN:"); false: there is none
static inline bool al_merge_field(const std::string &l, const char *pre, std::string *val)
{
	const size_t m = strlen(pre);
	for (size_t p = 0; p <= l.size(); ) { size_t q = l.find('\t', p); if (q == std::string::npos) q = l.size(); if (p && l.compare(p, m, pre) == 0) { *val = l.substr(p + m, q - p - m); return true; } p = q + 1; }
	return false;
}
static inline void al_merge_lines(const std::string &text, std::vector<std::string> &lines, std::string *tail)
{
	std::string t = text;
	{ const size_t z = t.find('\0'); if (z != std::string::npos) { if (tail) *tail = t.substr(z); t.resize(z); } }
	lines.clear();
	for (size_t p = 0; p < t.size(); ) { const size_t q = t.find('\n', p); if (q == std::string::npos) { lines.push_back(t.substr(p)); break; } lines.push_back(t.substr(p, q - p)); p = q + 1; }
}
// The output's header, reference list and the inputs' tables (REFERENCE LISTS and HEADER TEXT above).  0, or -1 with err set.
static inline int al_merge_headers(const std::vector<AlLiftHeader> &H, const std::vector<std::string> &fn, AlMergeHeaders &M, std::string &err)
{
	M = AlMergeHeaders();
	std::vector<std::string> out, lines; std::string tail;
	al_merge_lines(H[0].text, lines, &tail);
	bool any_hd = false;
	for (const std::string &l : lines) if (al_merge_is(l, "@HD")) any_hd = true;
	if (!any_hd) out.push_back("@HD\tVN:1.6\tSO:coordinate");
	for (const std::string &l : lines) out.push_back(al_merge_is(l, "@HD") ? al_lift_hd_line(l, true) : l);
	std::unordered_map<std::string, uint32_t> by_name; std::vector<size_t> origin;
	M.name = H[0].name; M.len = H[0].len; M.map.resize(H.size());
	for (size_t r = 0; r < M.name.size(); ++r) {
		if (by_name.count(M.name[r])) { err = "'" + fn[0] + "': contig '" + M.name[r] + "' is listed twice"; return -1; }
		by_name[M.name[r]] = (uint32_t)r; origin.push_back(0); M.map[0].push_back((int32_t)r);
	}
	for (size_t i = 1; i < H.size(); ++i) {
		std::vector<uint32_t> fresh;
		for (size_t r = 0; r < H[i].name.size(); ++r) {
			const std::string &nm = H[i].name[r];
			auto it = by_name.find(nm); uint32_t j;
			if (it == by_name.end()) { j = (uint32_t)M.name.size(); by_name[nm] = j; M.name.push_back(nm); M.len.push_back(H[i].len[r]); origin.push_back(i); fresh.push_back(j); }
			else {
				j = it->second;
				if (M.len[j] != H[i].len[r]) { err = "'" + fn[i] + "': contig '" + nm + "' has length " + std::to_string(H[i].len[r]) + " here and " + std::to_string(M.len[j]) + " in '" + fn[origin[j]] + "'"; return -1; }
			}
			if (r && (int32_t)j <= M.map[i][r - 1]) {
				err = "'" + fn[i] + "': contigs '" + H[i].name[r - 1] + "' and '" + nm + "' stand in the other order in the merged reference list: the input would not be in coordinate order there";
				return -1;
			}
			M.map[i].push_back((int32_t)j);
		}
		al_merge_lines(H[i].text, lines, nullptr);
		for (uint32_t j : fresh) {
			std::string sq = "@SQ\tSN:" + M.name[j] + "\tLN:" + std::to_string(M.len[j]), sn;
			for (const std::string &l : lines) if (al_merge_is(l, "@SQ") && al_merge_field(l, "SN:", &sn) && sn == M.name[j]) { sq = l; break; }
			out.push_back(sq);
		}
		for (const std::string &l0 : lines) {
			if (l0.empty() || al_merge_is(l0, "@HD") || al_merge_is(l0, "@SQ")) continue;
			if (al_merge_is(l0, "@CO")) { out.push_back(l0); continue; }
			bool same = false;
			for (const std::string &o : out) if (o == l0) { same = true; break; }
			if (same) continue;
			std::string l = l0, id, oid;
			const bool pg = al_merge_is(l, "@PG"), rg = al_merge_is(l, "@RG");
			if ((pg || rg) && al_merge_field(l, "ID:", &id)) {
				bool hit = false;
				for (const std::string &o : out) if (al_merge_is(o, pg ? "@PG" : "@RG") && al_merge_field(o, "ID:", &oid) && oid == id) { hit = true; break; }
				if (hit && rg) { err = "'" + fn[i] + "': the @RG line with ID '" + id + "' differs from the one already present: the records' RG:Z tags would have to be rewritten, which merge does not do"; return -1; }
				if (hit) { const size_t p = l.find("\tID:" + id); l.insert(p + 4 + id.size(), "." + std::to_string(i + 1)); }
			}
			out.push_back(l);
		}
	}
	std::string text;
	for (const std::string &l : out) { text += l; text += '\n'; }
	text += tail;
	auto p32 = [&](uint32_t v) { uint8_t b[4]; al_lift_p32(b, v); M.out.insert(M.out.end(), b, b + 4); };
	M.out.insert(M.out.end(), {'B', 'A', 'M', 1}); p32((uint32_t)text.size()); M.out.insert(M.out.end(), text.begin(), text.end()); p32((uint32_t)M.name.size());
	for (size_t i = 0; i < M.name.size(); ++i) { p32((uint32_t)M.name[i].size() + 1); M.out.insert(M.out.end(), M.name[i].begin(), M.name[i].end()); M.out.push_back(0); p32(M.len[i]); }
	for (auto &m : M.map) if (m.empty()) m.reserve(1);
	return 0;
}

// ---- the host twin of the per-record kernels -----------------------------------------------------------------------------------------------------------------------
// What k_merge_key and k_merge_descents compute over the n records at rec_off of the text t: key and rlen per record, *first_bad (~0: none) the first record with a
// refID beyond the list, *descents the positions whose key is below the key before them -- position 0 against prev_key when has_prev -- and *desc_off the
// smallest offset of such a record (~0: none).
static inline void al_merge_keys_host(uint8_t *t, const uint32_t *rec_off, size_t n, const int32_t *map, uint32_t n_ref, bool has_prev, uint64_t prev_key,
                                      uint64_t *key, uint32_t *rlen, uint64_t *first_bad, uint64_t *descents, uint64_t *desc_off)
{
	*first_bad = ~0ull; *descents = 0; *desc_off = ~0ull;
	for (size_t k = 0; k < n; ++k) {
		if (al_merge_record(t + rec_off[k], map, n_ref, &key[k], &rlen[k]) && *first_bad == ~0ull) *first_bad = k;
		const bool d = k ? key[k] < key[k - 1] : (has_prev && key[0] < prev_key);
		if (d) { ++*descents; if (rec_off[k] < *desc_off) *desc_off = rec_off[k]; }
	}
}

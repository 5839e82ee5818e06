// al_dev_chainexact.h -- `chain-exact verify|build`: the reference's run/1_build_exact_chain_file.py as ONE function of two texts and a block table, written
// once for both sides: the pieces below are compiled for the device (k_cex_fold, k_cex_count, k_cex_emit, k_cex_lines, the pass-2 scan: al_chainexact.hip) and
// for the CPU (the twin in this file, which evaluates the same function serially, the way the script does).  The twin is what the kernels are tested against,
// what `chain-exact --host` runs and what tests/csrc/chainexact_main.cpp runs under the sanitizers.
//
// In the script "source" is the OLD reference (header fields tName .. tEnd) and "target" the NEW one (qName .. qEnd).
//
// PARSING (host, al_cex_parse).  As al_chn_parse of al_dev_chainreg.h, and it keeps the q side: qName, qSize, qStrand ('+' or '-'), qStart, every line's dq and
// the header's tokens as written (12 without an id, or 13).  Refused, as FILE:LINE: reason: what al_chn_parse refuses (tStrand must be '+'), a header number
// that is none, a chain whose last line is not 1-field, two headers with the same (tName, qName, tStart).
//
// ORDER OF CHAINS.  The script nests dicts: chains come out by first appearance of tName, inside that of qName, inside that of tStart -- a stable sort of the
// headers by those three ranks (AlCexTab::order, made at the end of al_cex_parse).
//
// THE TABLE (host, al_cex_table).  Blocks in output order, {chain, size, dt, dq, three}; per chain old0 / new0, the text offsets of its first block's first
// base (new0: of qSize - qStart - 1 on a '-' chain), and dir.  verify: a chain whose tName or qName its FASTA lacks is left out; inside a chain the first
// block with L_old < sfrom + size + 1 (on '+' also L_new < tfrom + size + 1) and everything behind it is left out (the script's rule as written: a block
// that ends on the contig's last base is not checked).  build: a missing name or a block that ends beyond L_old / L_new is refused.  On a '-' chain a block
// whose new-side indices leave [0, L_new) is refused.
//
// THE FUNCTION.  Blocks i = 0..n-1:
//  1. old_off[i] = old0 + sum of size + dt over the earlier blocks of the chain, new_off[i] = new0 +/- sum of size + dq: one segmented scan of pairs
//     (al_cex_sum_op).
//  2. Base idx of block i mismatches when lower(old[old_off + idx]) != lower(new[new_off + idx]) ('+') or != comp(lower(new[new_off - idx])) ('-');
//     lower changes only A-Z, comp maps a<->t, c<->g, n<->n and raises the error flag for any other byte.  cnt[i], and the positions {block, idx} in order.
//  3. Pass-1 lines: mismatch number m (counted over all blocks) of block b is line m + b, "gap-before 1 1"; block b's closing line is at (first mismatch
//     number of block b + 1) + b: "size - last - 1 [dt dq]", or the block's line as it is without a mismatch (al_cex_line_mis, al_cex_line_close).
//  4. Pass 2, per chain, M = --min-region: a line is KEPT when it is 1-field or size >= M.  Every kept line and every chain's first line heads a segment;
//     a segment is one output line: the head's size (0 when the head is a small line in front of the chain's first kept line), and dt / dq = the sums over
//     the segment of (dt, dq) for the kept head and (size + dt, size + dq) for every small line (al_cex_p2_elem, al_cex_sum_op again).  The twin runs the
//     script's state machine instead; they are the same lines.
//  5. Pass 3 and the printing (host, al_cex_build_text): a leading "0 s t" line is dropped, tStart += s, qStart += t; a last line "0" is dropped, its 3-field
//     predecessor "z s t" becomes "z", tEnd -= s, qEnd -= t.  A header that changes prints qStart and qEnd as integers (the script re-formats both).
#pragma once
#include "al_dev_chainreg.h"      // AL_DHD, al_chn_fields, al_chn_num, AlChnLineReader
#include <map>

#define AL_CEX_TILE 4096u         // bases of a block that one wavefront compares
#define AL_CEX_VERIFY 0
#define AL_CEX_BUILD 1
#define AL_CEX_MOST 0x7ffffff0ull // blocks, tiles, mismatches and lines of one run

struct alignas(16) AlCexLine { uint32_t chain, size, dt, dq, three, pad[3]; };
struct alignas(16) AlCexChain { uint64_t old0, new0; uint32_t dir, pad[3]; };
struct AlCexPos { uint32_t block, idx; };
struct alignas(16) AlCexSum { uint64_t a, b; };                           // a: bit 63 = a segment starts at (or inside) what the element covers

AL_DHD uint8_t al_cex_lower(uint8_t c) { return c >= 'A' && c <= 'Z' ? (uint8_t)(c | 0x20) : c; }
AL_DHD uint8_t al_cex_comp(uint8_t c)                                     // of a folded byte; 0xff: none
{
	return c == 'a' ? 't' : c == 't' ? 'a' : c == 'c' ? 'g' : c == 'g' ? 'c' : c == 'n' ? 'n' : 0xff;
}
#define AL_CEX_F (1ull << 63)
AL_DHD AlCexSum al_cex_sum_elem(bool seg_start, uint64_t va, uint64_t vb) { return AlCexSum{(seg_start ? AL_CEX_F : 0ull) | va, vb}; }
AL_DHD AlCexSum al_cex_sum_op(const AlCexSum &x, const AlCexSum &y)
{
	if (y.a & AL_CEX_F) return y;
	return AlCexSum{(x.a & AL_CEX_F) | (((x.a & ~AL_CEX_F) + y.a) & ~AL_CEX_F), x.b + y.b};
}
AL_DHD AlCexSum al_cex_off_elem(const AlCexLine *l, uint64_t i) { return al_cex_sum_elem(i == 0 || l[i - 1].chain != l[i].chain, (uint64_t)l[i].size + l[i].dt, (uint64_t)l[i].size + l[i].dq); }
// block i's first base in both texts from the inclusive sums
AL_DHD void al_cex_off(const AlCexLine &l, const AlCexChain &c, const AlCexSum &s, uint64_t *old_off, uint64_t *new_off)
{
	const uint64_t a = (s.a & ~AL_CEX_F) - ((uint64_t)l.size + l.dt), b = s.b - ((uint64_t)l.size + l.dq);
	*old_off = c.old0 + a; *new_off = c.dir ? c.new0 - b : c.new0 + b;
}
AL_DHD AlCexLine al_cex_mk(uint32_t chain, uint32_t size, uint32_t dt, uint32_t dq, uint32_t three) { AlCexLine l{}; l.chain = chain; l.size = size; l.dt = dt; l.dq = dq; l.three = three; return l; }
// pass 1: the line of mismatch m (`first`: the number of its block's first mismatch), and a block's closing line
AL_DHD AlCexLine al_cex_line_mis(const AlCexLine &blk, const AlCexPos *pos, uint64_t m, uint64_t first)
{
	return al_cex_mk(blk.chain, m == first ? pos[m].idx : pos[m].idx - pos[m - 1].idx - 1, 1, 1, 1);
}
AL_DHD AlCexLine al_cex_line_close(const AlCexLine &blk, const AlCexPos *pos, uint64_t first, uint64_t next_first)
{
	return al_cex_mk(blk.chain, next_first > first ? blk.size - pos[next_first - 1].idx - 1 : blk.size, blk.dt, blk.dq, blk.three);
}
// pass 2
AL_DHD bool al_cex_kept(const AlCexLine &l, uint32_t M) { return !l.three || l.size >= M; }
AL_DHD bool al_cex_p2_head(const AlCexLine *l, uint64_t i, uint32_t M) { return i == 0 || l[i - 1].chain != l[i].chain || al_cex_kept(l[i], M); }
AL_DHD AlCexSum al_cex_p2_elem(const AlCexLine *l, uint64_t i, uint32_t M)
{
	const AlCexLine &x = l[i];
	const bool kept = al_cex_kept(x, M);
	const uint64_t add = kept ? 0 : x.size;
	return al_cex_sum_elem(al_cex_p2_head(l, i, M), x.three ? add + x.dt : 0, x.three ? add + x.dq : 0);
}
AL_DHD AlCexLine al_cex_p2_out(const AlCexLine &h, uint32_t M) { return al_cex_mk(h.chain, al_cex_kept(h, M) ? h.size : 0, 0, 0, h.three); }

// what the function is evaluated on
struct AlCexIn {
	const uint8_t *old_text = nullptr, *new_text = nullptr; uint64_t n_old = 0, n_new = 0;
	uint64_t n = 0; const AlCexLine *line = nullptr;
	uint32_t n_chain = 0; const AlCexChain *chain = nullptr;
};
// what it gives; the device form fills pos / lines1 only when asked (the test taps)
struct AlCexOut {
	std::vector<uint32_t> cnt; std::vector<AlCexPos> pos; std::vector<AlCexLine> lines1, lines2; uint32_t flag = 0;
	double ms_kernels = 0, ms_fold = 0, ms_count = 0, ms_emit = 0, ms_h2d = 0; uint64_t bytes_h2d = 0, bytes_d2h = 0;
};

// what al_cex_table guarantees of a table, checked where a table comes from elsewhere (the test taps): null, or what is wrong.  build: pass 2 is wanted
static inline const char *al_cex_in_bad(const AlCexIn &in, bool build)
{
	if (in.n >= AL_CEX_MOST) return "more blocks than a run takes";
	if ((in.n_old && !in.old_text) || (in.n_new && !in.new_text) || (in.n && !in.line) || (in.n_chain && !in.chain)) return "a table is missing";
	uint64_t a = 0, b = 0, tiles = 0;
	for (uint64_t i = 0; i < in.n; ++i) {
		const AlCexLine &l = in.line[i];
		if (l.chain >= in.n_chain || (i && l.chain < in.line[i - 1].chain)) return "a block's chain lies outside the table or before the block's predecessor's";
		if (i == 0 || l.chain != in.line[i - 1].chain) a = b = 0;
		if (l.size == 0 || (!l.three && (l.dt || l.dq)) || l.three > 1) return "a block has size 0, or gaps without three fields";
		const AlCexChain &c = in.chain[l.chain];
		if (c.dir > 1) return "a chain's direction is neither 0 nor 1";
		if (c.old0 + a + l.size > in.n_old) return "a block ends beyond the old text";
		if (!c.dir && c.new0 + b + l.size > in.n_new) return "a block ends beyond the new text";
		if (c.dir && (c.new0 >= in.n_new || b > c.new0 || c.new0 - b + 1 < l.size)) return "a '-' block leaves the new text";
		a += (uint64_t)l.size + l.dt; b += (uint64_t)l.size + l.dq;
		if (a > 0xffffffffull || b > 0xffffffffull) return "a chain's blocks and gaps span 2^32 bases or more";
		tiles += (l.size + AL_CEX_TILE - 1) / AL_CEX_TILE;
		const bool last = i + 1 == in.n || in.line[i + 1].chain != l.chain;
		if (build && (last ? l.three != 0 : l.three == 0)) return "a chain's last line, and only that, is 1-field";
	}
	if (tiles >= AL_CEX_MOST) return "more tiles than a run takes";
	return nullptr;
}

// ---- the host twin -------------------------------------------------------------------------------------------------------------------------------------------
// counts and, when want_pos, positions; the error flag
static inline void al_cex_compare_host(const AlCexIn &in, bool want_pos, AlCexOut &o)
{
	o.cnt.assign(in.n, 0); o.pos.clear(); o.flag = 0;
	AlCexSum acc{0, 0};
	for (uint64_t i = 0; i < in.n; ++i) {
		const AlCexLine &l = in.line[i]; const AlCexChain &c = in.chain[l.chain];
		acc = al_cex_sum_op(acc, al_cex_off_elem(in.line, i));
		uint64_t oo, no; al_cex_off(l, c, acc, &oo, &no);
		const uint8_t *a = in.old_text + oo; uint32_t k = 0;
		if (!c.dir) {
			const uint8_t *b = in.new_text + no;
			for (uint32_t idx = 0; idx < l.size; ++idx)
				if (a[idx] != b[idx] && al_cex_lower(a[idx]) != al_cex_lower(b[idx])) { ++k; if (want_pos) o.pos.push_back(AlCexPos{(uint32_t)i, idx}); }
		} else {
			for (uint32_t idx = 0; idx < l.size; ++idx) {
				const uint8_t r = al_cex_comp(al_cex_lower(in.new_text[no - idx]));
				if (r == 0xff) o.flag = 1;
				if (al_cex_lower(a[idx]) != r) { ++k; if (want_pos) o.pos.push_back(AlCexPos{(uint32_t)i, idx}); }
			}
		}
		o.cnt[i] = k;
	}
}
static inline void al_cex_lines1_host(const AlCexIn &in, AlCexOut &o)
{
	o.lines1.clear();
	uint64_t m = 0;
	for (uint64_t i = 0; i < in.n; ++i) {
		const uint64_t first = m;
		for (; m < first + o.cnt[i]; ++m) o.lines1.push_back(al_cex_line_mis(in.line[i], o.pos.data(), m, first));
		o.lines1.push_back(al_cex_line_close(in.line[i], o.pos.data(), first, m));
	}
}
// the script's second pass, as it is written
static inline void al_cex_pass2_host(const std::vector<AlCexLine> &l1, uint32_t M, std::vector<AlCexLine> &l2)
{
	l2.clear();
	int64_t last_size = -1; uint64_t sg = 0, tg = 0;
	for (size_t i = 0; i < l1.size(); ++i) {
		const AlCexLine &l = l1[i];
		if (i == 0 || l1[i - 1].chain != l.chain) { last_size = -1; sg = tg = 0; }
		if (l.three) {
			if (l.size < M) { sg += (uint64_t)l.dt + l.size; tg += (uint64_t)l.dq + l.size; if (last_size == -1) last_size = 0; }
			else {
				if (last_size != -1) l2.push_back(al_cex_mk(l.chain, (uint32_t)last_size, (uint32_t)sg, (uint32_t)tg, 1));
				sg = l.dt; tg = l.dq; last_size = l.size;
			}
		} else {
			if (last_size != -1) l2.push_back(al_cex_mk(l.chain, (uint32_t)last_size, (uint32_t)sg, (uint32_t)tg, 1));
			l2.push_back(al_cex_mk(l.chain, l.size, 0, 0, 0));
		}
	}
}
// the whole function on the twin; build: positions and both line lists too
static inline void al_chainexact_host(const AlCexIn &in, bool build, uint32_t M, AlCexOut &o)
{
	al_cex_compare_host(in, build, o);
	o.lines1.clear(); o.lines2.clear();
	if (build && !o.flag) { al_cex_lines1_host(in, o); al_cex_pass2_host(o.lines1, M, o.lines2); }
}

// ---- the chain file ------------------------------------------------------------------------------------------------------------------------------------------
struct AlCexHdr {
	std::vector<std::string> tok;                                         // as written
	uint32_t tslot = 0, qrank = 0; uint64_t tsize = 0, tstart = 0, qsize = 0, qstart = 0; bool minus = false;
	unsigned long long line_no = 0; uint64_t first = 0, n = 0;            // its alignment lines in AlCexTab::line
};
struct AlCexFLine { uint32_t size, dt, dq, three; unsigned long long line_no; };
struct AlCexTab { std::vector<std::string> tname; std::vector<uint32_t> L; std::vector<AlCexHdr> hdr; std::vector<AlCexFLine> line; std::vector<uint32_t> order; };

static inline bool al_cex_score_ok(const char *s, size_t n)
{
	size_t i = n && (s[0] == '-' || s[0] == '+') ? 1 : 0;
	if (i >= n) return false;
	for (; i < n; ++i) if (s[i] < '0' || s[i] > '9') return false;
	return true;
}
// 0, or -1 with err = "FILE:LINE: reason" (or "FILE: reason")
static inline int al_cex_parse(const char *fn, AlCexTab &t, std::string &err)
{
	AlChnLineReader rd;
	if (!rd.open(fn)) { err = std::string(fn) + ": cannot be opened"; return -1; }
	auto fail_at = [&](unsigned long long ln, const char *why) { err = std::string(fn) + ":" + std::to_string(ln) + ": " + why; return -1; };
	auto fail = [&](const char *why) { return fail_at(rd.n_line, why); };
	std::vector<std::pair<size_t, size_t>> f;
	std::unordered_map<std::string, uint32_t> by_name;
	std::map<std::pair<uint32_t, std::string>, uint32_t> q_rank; std::vector<uint32_t> n_q;
	std::map<std::pair<std::pair<uint32_t, uint32_t>, uint64_t>, int> seen;
	const char *l; size_t n; bool have = false, closed = false; uint64_t pos = 0; uint32_t slot = 0;
	auto close_chain = [&]() -> int {
		if (!have) return 0;
		const AlCexHdr &h = t.hdr.back();
		if (h.n == 0) return fail_at(h.line_no, "a chain without alignment lines");
		if (t.line.back().three) return fail_at(t.line.back().line_no, "the chain's last line is not 1-field");
		return 0;
	};
	while (rd.next(&l, &n)) {
		if (n && l[0] == '#') continue;
		al_chn_fields(l, n, f, 64);
		if (f.empty()) continue;
		if (f[0].second == 5 && !memcmp(l + f[0].first, "chain", 5)) {
			if (close_chain()) return -1;
			if (f.size() < 12) return fail("a chain header with fewer than 12 fields");
			if (f.size() > 13) return fail("a chain header with more than 13 fields");
			AlCexHdr h; uint64_t tend, qend;
			if (!al_cex_score_ok(l + f[1].first, f[1].second)) return fail("the score is not a number");
			if (!al_chn_num(l + f[3].first, f[3].second, &h.tsize)) return fail("tSize is not a number");
			if (!al_chn_num(l + f[5].first, f[5].second, &h.tstart)) return fail("tStart is not a number");
			if (!al_chn_num(l + f[6].first, f[6].second, &tend)) return fail("tEnd is not a number");
			if (!al_chn_num(l + f[8].first, f[8].second, &h.qsize)) return fail("qSize is not a number");
			if (!al_chn_num(l + f[10].first, f[10].second, &h.qstart)) return fail("qStart is not a number");
			if (!al_chn_num(l + f[11].first, f[11].second, &qend)) return fail("qEnd is not a number");
			if (h.tsize >= (1ull << 31)) return fail("tSize is 2^31 or more");
			if (h.qsize >= (1ull << 31)) return fail("qSize is 2^31 or more");
			if (f[4].second != 1 || l[f[4].first] != '+') return fail("tStrand is not '+'");
			if (f[9].second != 1 || (l[f[9].first] != '+' && l[f[9].first] != '-')) return fail("qStrand is neither '+' nor '-'");
			h.minus = l[f[9].first] == '-';
			for (const auto &x : f) h.tok.push_back(std::string(l + x.first, x.second));
			auto it = by_name.find(h.tok[2]);
			if (it == by_name.end()) { slot = (uint32_t)t.tname.size(); by_name[h.tok[2]] = slot; t.tname.push_back(h.tok[2]); t.L.push_back((uint32_t)h.tsize); n_q.push_back(0); }
			else slot = it->second;                                          // (a later header's tSize changes nothing, as in al_chn_parse)
			if (h.tstart > t.L[slot]) return fail("tStart lies beyond tSize");
			if (t.hdr.size() >= 0xfffffff0u) return fail("more chains than a run takes");
			auto qi = q_rank.find({slot, h.tok[7]});
			if (qi == q_rank.end()) { h.qrank = n_q[slot]++; q_rank[{slot, h.tok[7]}] = h.qrank; } else h.qrank = qi->second;
			if (seen[{{slot, h.qrank}, h.tstart}]++) return fail("a second header with the same tName, qName and tStart");
			h.tslot = slot; h.line_no = rd.n_line; h.first = t.line.size();
			t.hdr.push_back(h);
			pos = h.tstart; have = true; closed = false;
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
		if (v[2] >= (1ull << 31)) return fail("dq is 2^31 or more");
		if (t.line.size() >= AL_CEX_MOST) return fail("more alignment lines than a run takes");
		t.line.push_back(AlCexFLine{(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], f.size() == 3 ? 1u : 0u, rd.n_line});
		++t.hdr.back().n;
		pos += v[0] + v[1];
		if (f.size() == 1) closed = true;
	}
	if (close_chain()) return -1;
	// the script's order: first appearance of tName, of qName inside it, of tStart inside that (distinct, so: file order)
	t.order.resize(t.hdr.size());
	for (uint32_t i = 0; i < t.order.size(); ++i) t.order[i] = i;
	std::stable_sort(t.order.begin(), t.order.end(), [&](uint32_t a, uint32_t b) {
		const AlCexHdr &x = t.hdr[a], &y = t.hdr[b];
		return x.tslot != y.tslot ? x.tslot < y.tslot : x.qrank < y.qrank;
	});
	return 0;
}

// a FASTA as the function sees it: names, offsets into one text, lengths
struct AlCexFa {
	std::vector<std::string> name; std::vector<uint64_t> off; std::vector<uint32_t> len; const uint8_t *text = nullptr; uint64_t n = 0;
	std::unordered_map<std::string, uint32_t> by_name;
	// null, or the name that appears twice
	const std::string *index() { by_name.clear(); for (uint32_t i = 0; i < name.size(); ++i) if (!by_name.emplace(name[i], i).second) return &name[i]; return nullptr; }
};
// the table of a run; chain c of it is header tab.order[c].  0, or -1 with err
struct AlCexRun { std::vector<AlCexLine> line; std::vector<AlCexChain> chain; std::vector<unsigned long long> line_no; };
static inline int al_cex_table(const char *chain_fn, const AlCexTab &t, const AlCexFa &fo, const AlCexFa &fn, int mode, AlCexRun &r, std::string &err)
{
	auto fail = [&](unsigned long long ln, const std::string &why) { err = std::string(chain_fn) + ":" + std::to_string(ln) + ": " + why; return -1; };
	r.line.clear(); r.chain.assign(t.order.size(), AlCexChain{}); r.line_no.clear();
	for (uint32_t c = 0; c < t.order.size(); ++c) {
		const AlCexHdr &h = t.hdr[t.order[c]];
		auto io = fo.by_name.find(h.tok[2]), in = fn.by_name.find(h.tok[7]);
		if (io == fo.by_name.end() || in == fn.by_name.end()) {
			if (mode == AL_CEX_VERIFY) continue;
			return fail(h.line_no, io == fo.by_name.end() ? "the old FASTA has no contig '" + h.tok[2] + "'" : "the new FASTA has no contig '" + h.tok[7] + "'");
		}
		const int64_t Lo = fo.len[io->second], Ln = fn.len[in->second];
		int64_t sfrom = (int64_t)h.tstart, tfrom = h.minus ? (int64_t)h.qsize - (int64_t)h.qstart - 1 : (int64_t)h.qstart;
		r.chain[c].old0 = fo.off[io->second] + (uint64_t)sfrom; r.chain[c].dir = h.minus ? 1u : 0u;
		r.chain[c].new0 = tfrom >= 0 ? fn.off[in->second] + (uint64_t)tfrom : 0;
		for (uint64_t i = h.first; i < h.first + h.n; ++i) {
			const AlCexFLine &l = t.line[i];
			const int64_t size = l.size;
			if (mode == AL_CEX_VERIFY) { if (Lo < sfrom + size + 1 || (!h.minus && Ln < tfrom + size + 1)) break; }
			else if (Lo < sfrom + size || (!h.minus && Ln < tfrom + size)) return fail(l.line_no, Lo < sfrom + size ? "the block ends beyond the old contig" : "the block ends beyond the new contig");
			if (h.minus && (tfrom >= Ln || tfrom - (size - 1) < 0)) return fail(l.line_no, "the block of a '-' chain leaves the new contig");
			r.line.push_back(al_cex_mk(c, l.size, l.dt, l.dq, l.three)); r.line_no.push_back(l.line_no);
			sfrom += size + l.dt; tfrom += h.minus ? -(size + (int64_t)l.dq) : size + (int64_t)l.dq;
		}
	}
	if (r.line.size() >= AL_CEX_MOST) { err = std::string(chain_fn) + ": more blocks than a run takes"; return -1; }
	return 0;
}
// the line of the first '-' block that compares a new-side byte other than acgtnACGTN (the error flag's where), or 0
static inline unsigned long long al_cex_flag_line(const AlCexIn &in, const AlCexRun &r)
{
	AlCexSum acc{0, 0};
	for (uint64_t i = 0; i < in.n; ++i) {
		const AlCexLine &l = in.line[i]; const AlCexChain &c = in.chain[l.chain];
		acc = al_cex_sum_op(acc, al_cex_off_elem(in.line, i));
		if (!c.dir) continue;
		uint64_t oo, no; al_cex_off(l, c, acc, &oo, &no);
		for (uint32_t idx = 0; idx < l.size; ++idx) if (al_cex_comp(al_cex_lower(in.new_text[no - idx])) == 0xff) return r.line_no[i];
	}
	return 0;
}

// ---- the text ------------------------------------------------------------------------------------------------------------------------------------------------
static inline void al_cex_join(std::string &o, const std::vector<std::string> &tok, char sep) { for (size_t i = 0; i < tok.size(); ++i) { if (i) o += sep; o += tok[i]; } }
// verify: a line per block with mismatches, or PASS VERIFICATION
static inline void al_cex_verify_text(const AlCexTab &t, const AlCexRun &r, const std::vector<uint32_t> &cnt, std::string &o)
{
	bool any = false; char num[96];
	for (size_t i = 0; i < r.line.size(); ++i) {
		if (!cnt[i]) continue;
		const AlCexHdr &h = t.hdr[t.order[r.line[i].chain]];
		o.append(num, (size_t)snprintf(num, sizeof(num), "mismatch: %u errors in %u blocktarget: ", cnt[i], r.line[i].size));
		o += h.tok[7]; o += " header: "; al_cex_join(o, h.tok, ' '); o += '\n';
		any = true;
	}
	if (!any) o += "PASS VERIFICATION\n";
}
// build: pass 3 over the lines of pass 2, and the printing
static inline void al_cex_build_text(const AlCexTab &t, const std::vector<AlCexLine> &l2, std::string &o)
{
	size_t i = 0; char num[64];
	auto dec = [](long long v) { return std::to_string(v); };
	for (uint32_t c = 0; c < t.order.size(); ++c) {
		const AlCexHdr &h = t.hdr[t.order[c]];
		size_t a = i; while (i < l2.size() && l2[i].chain == c) ++i;
		size_t b = i;                                                       // this chain's lines [a, b); the last is 1-field
		std::vector<std::string> tok = h.tok;
		const long long qs = atoll(tok[10].c_str()), qe = atoll(tok[11].c_str());
		if (a < b && l2[a].three && l2[a].size == 0) {
			tok[5] = dec((long long)h.tstart + l2[a].dt); tok[10] = dec(qs + l2[a].dq); tok[11] = dec(qe);
			++a;
		}
		bool strip = false;                                                  // the line in front of a dropped "0" loses its gaps
		if (a < b && !l2[b - 1].three && l2[b - 1].size == 0) {
			--b;
			if (a < b) {
				tok[6] = dec(atoll(tok[6].c_str()) - (long long)l2[b - 1].dt);
				tok[10] = dec(atoll(tok[10].c_str())); tok[11] = dec(qe - (long long)l2[b - 1].dq);
				strip = true;
			}
		}
		if (c) o += '\n';
		al_cex_join(o, tok, '\t'); o += '\n';
		for (size_t k = a; k < b; ++k) {
			if (l2[k].three && !(strip && k + 1 == b)) o.append(num, (size_t)snprintf(num, sizeof(num), "%u\t%u\t%u\n", l2[k].size, l2[k].dt, l2[k].dq));
			else o.append(num, (size_t)snprintf(num, sizeof(num), "%u\n", l2[k].size));
		}
	}
}

// ---- the device form (al_chainexact.hip) -----------------------------------------------------------------------------------------------------------------------
// Uploads both texts (one byte per base, exactly their size) and the table, folds the texts, counts, and for build emits the positions, makes the pass-1 lines
// and folds them (pass 2); only the counts, the flag and the folded lines come back -- the positions and the pass-1 lines too when `taps`.  Every device
// buffer is obtained through al_dev_malloc and released before it returns.
int al_chainexact_device(int device, const AlCexIn &in, bool build, uint32_t M, bool taps, AlCexOut &o);

// al_bai.h -- the driver of `bam-index`: the record stream of one coordinate-sorted BAM walked in pieces, the function of al_dev_bai.h evaluated by a backend, the
// runs' rows and the per-contig tables made into the BAI by host code both backends share.  Host code only, no HIP include: the device backend lives in
// al_bai.hip, the host backend (the twin) is at the end of this file, and tests/csrc/index_main.cpp runs this loop with the twin under the sanitizers.  Modelled
// on al_merge.h.
//
// The loop is merge's for a single input: the carry of the incomplete tail, the next piece, inflate, walk, keys; a piece without a complete record doubles the
// next one.  The driver keeps the table of the BGZF members that overlap the current text -- the port through which the source appends notes every member it
// passes on -- and hands it to the backend with each piece.  A backend holds two texts that take turns, and the per-contig tables (AlBaiTables) from the first
// piece to the last; per piece it returns the refusals and the rows of the runs, the last of which stays open: the driver joins it to the next piece's first run
// when (refID, bin) match, and sets its end when that was not known yet (AL_BAI_OPEN).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <unistd.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <vector>
#include "al_dev_bai.h"
#include "al_lift.h"               // lift_read_header, al_lift_malformed, al_lift_walk_host; al_bgzf_take.h

struct AlBaiPiece {
	uint64_t n_rec = 0, consumed = 0; uint32_t walk_bad = 0;          // complete records from the start offset on, offset of the first incomplete one, its block_size is out of range
	uint64_t first_bad = ~0ull; uint32_t bad_code = 0; uint64_t bad_off = 0;   // the first record al_bai_record refuses: its number, code and offset
	uint64_t descents = 0, desc_off = ~0ull, last_key = 0;            // records below their predecessor, the smallest offset of one; the key of the last record
};
struct AlBaiRun { uint64_t pieces = 0, bytes_in = 0, records = 0, unplaced = 0, chunks = 0, bai_bytes = 0; double read_s = 0, up_s = 0, inflate_s = 0, walk_s = 0, key_s = 0, assemble_s = 0; };

struct AlBaiBackend {
	virtual ~AlBaiBackend() {}
	virtual const char *name() const = 0;
	virtual int set_refs(const uint32_t *len, uint32_t n_ref) = 0;                        // the header's contig lengths, before the first run(): the tables are made
	virtual int begin(size_t cap) = 0;                                                    // the other text: empty, room for cap bytes; it is the current one from here on
	virtual int carry(uint64_t off, uint64_t n) = 0;                                      // bytes [off, off + n) of the text that was current before begin(), appended
	virtual int append(const uint8_t *p, size_t n) = 0;                                   // host bytes appended
	virtual int append_bgzf(const uint8_t *bytes, size_t n_in, const AlInfMember *mem, size_t n_mem, uint64_t n_out, size_t *bad, uint32_t *bad_status) = 0;   // whole members inflated to the text's end; 1: *bad has a status
	virtual uint64_t text_bytes() const = 0;
	// walk from `start`; keys, runs, the tables' share.  base: the stream offset of the text's first byte; mem: the members that overlap the text
	virtual int run(uint64_t start, uint64_t base, const AlBaiMember *mem, size_t n_mem, bool has_prev, uint64_t prev_key, AlBaiPiece *r, std::vector<AlBaiRow> &rows) = 0;
	virtual int tables(AlBaiTables &T) = 0;                                               // after the last piece: lin and cnt (ref_len and lin_off as set_refs made them)
	virtual void *host_buffer(size_t bytes) = 0;                                          // page-locked on the device backend; nullptr: none
	virtual void host_buffer_free(void *p) = 0;
	virtual void stat(AlBaiRun &) {}                                                      // adds the backend's seconds
	virtual size_t held() const { return 0; }                                             // device bytes of the backend's account
};

// ---- what the driver keeps between the pieces --------------------------------------------------------------------------------------------------------------------
struct AlBaiAcc {
	std::vector<AlBaiMember> tab;                                      // the members that overlap the current text
	uint64_t after_last = 0;                                           // the file offset behind the last non-empty member seen
	std::vector<AlBaiRow> rows;                                        // the closed runs with refID >= 0, in file order
	AlBaiRow open = {-1, 0, 0, 0}; bool has_open = false, pending = false; uint64_t pend_s = 0;   // the last run; pending: its end is the offset of stream offset pend_s, not known yet
	void member(uint64_t s_off, uint64_t file_off, uint32_t isize, uint32_t msize) { tab.push_back(AlBaiMember{s_off, file_off, isize, msize}); if (isize) after_last = file_off + msize; }
	void prune(uint64_t base) { size_t k = 0; while (k < tab.size() && tab[k].s_off + tab[k].isize <= base) ++k; tab.erase(tab.begin(), tab.begin() + (ptrdiff_t)k); }
	void resolve(bool eof)
	{
		if (!pending) return;
		uint64_t v = al_bai_voff(tab.data(), (uint32_t)tab.size(), pend_s);
		if (v == AL_BAI_OPEN && eof) v = after_last << 16;
		if (v != AL_BAI_OPEN) { open.end = v; pending = false; }
	}
	void flush() { if (has_open && open.ref >= 0) rows.push_back(open); has_open = false; }
	// a piece's rows; text_end: the stream offset behind the piece's text, where a record whose end is open ends
	void add(const std::vector<AlBaiRow> &r, uint64_t text_end)
	{
		for (size_t i = 0; i < r.size(); ++i) {
			if (i == 0 && has_open && r[0].ref >= 0 && r[0].ref == open.ref && r[0].bin == open.bin) open.end = r[0].end;
			else { flush(); open = r[i]; has_open = true; }
		}
		if (!r.empty() && open.end == AL_BAI_OPEN) { pending = true; pend_s = text_end; }
	}
};

// what AlBgzfPieceSource takes for a backend: the bytes go on to the backend, the members are noted on the way
struct AlBaiPort {
	AlBaiBackend *B = nullptr; AlBaiAcc *A = nullptr; uint64_t s_at = 0, f_at = 0;        // stream and file offset of the next member
	int append(int, const uint8_t *p, size_t n) { return B->append(p, n); }
	int append_bgzf(int, const uint8_t *bytes, size_t n_in, const AlInfMember *mem, size_t n_mem, uint64_t n_out, size_t *bad, uint32_t *bad_status)
	{
		for (size_t k = 0; k < n_mem; ++k) A->member(s_at + mem[k].out_off, f_at + mem[k].in_off, mem[k].isize, mem[k].msize);
		s_at += n_out; f_at += n_in;
		return B->append_bgzf(bytes, n_in, mem, n_mem, n_out, bad, bad_status);
	}
	void *host_buffer(size_t n) { return B->host_buffer(n); }
	void host_buffer_free(void *p) { B->host_buffer_free(p); }
};
struct AlBaiSource {
	virtual ~AlBaiSource() {}
	virtual int read(int slot, size_t want) = 0;                       // 0, or -1 with a message printed (slot is always 0 here)
	virtual int push(AlBaiPort &B, int slot, bool *eof) = 0;           // what read() brought; *eof: the stream has ended with it
	virtual size_t pending(int slot) const = 0;                        // upper bound of the text bytes push() will append
	double read_s = 0;
	typedef AlLiftSource::Timer Timer;
};
// BGZF file from a member's file offset on
struct AlBaiBgzfSource : AlBgzfPieceSource<AlBaiPort, AlBaiSource> { AlBaiBgzfSource() { tag = "bam-index"; } };
// an uncompressed stream in memory with the table of the members it would lie in (the taps, tests/csrc/index_main.cpp): a member is noted with its first byte
struct AlBaiMemSource : AlBaiSource {
	const uint8_t *p = nullptr; size_t n = 0, at = 0, want = 0;
	const uint64_t *m_file = nullptr, *m_stream = nullptr; const uint32_t *m_isize = nullptr; size_t n_mem = 0, m_at = 0; uint64_t file_end = 0;
	int read(int, size_t w) override { want = w; return 0; }
	size_t pending(int) const override { return std::min(want, n - at); }
	int push(AlBaiPort &B, int, bool *eof) override
	{
		const size_t m = std::min(want, n - at);
		if (B.append(0, p + at, m)) return -1;
		at += m; *eof = at == n;
		for (; m_at < n_mem && (m_stream[m_at] < at || *eof); ++m_at) B.A->member(m_stream[m_at], m_file[m_at], m_isize[m_at], (uint32_t)((m_at + 1 < n_mem ? m_file[m_at + 1] : file_end) - m_file[m_at]));
		return 0;
	}
};

static inline int al_bai_refused(const char *fn, uint64_t off, uint32_t code)
{
	if (code == AL_BAI_BAD_BIG) fprintf(stderr, "ERROR: '%s': the record at offset %llu of the inflated stream ends beyond 2^29: the BAI format ends there, and a CSI index is not built\n", fn, (unsigned long long)off);
	else if (code == AL_BAI_BAD_LN) fprintf(stderr, "ERROR: '%s': the record at offset %llu of the inflated stream ends beyond its contig's length (LN): the linear index has no window there\n", fn, (unsigned long long)off);
	else return al_lift_malformed(fn, off, code);
	return -2;
}

// The records of one stream through the backend.  The first text's records start at offset `start` of it; base: the stream offset of that text's first byte.
// 0 with A.rows complete; -1 with a message printed; -2 refused input, its message printed.
static inline int al_bai_stream(AlBaiBackend &B, AlBaiSource &src, AlBaiPort &port, size_t piece, uint64_t start, uint64_t base, const char *fn, AlBaiAcc &A, AlBaiRun &st)
{
	size_t want = piece ? piece : 1; bool first = true, eof = false, has_prev = false; uint64_t prev_key = 0, consumed = 0; std::vector<AlBaiRow> rows;
	for (;;) {
		const uint64_t tail = first ? 0 : B.text_bytes() - consumed;
		if (src.read(0, want)) return -1;
		const size_t pend = src.pending(0);
		if (tail + pend + 1 >= (1ull << 31)) { fprintf(stderr, "[ERROR] airlift: bam-index: '%s': a text of more than 2 GB\n", fn); return -1; }
		if (B.begin((size_t)tail + pend + 1) || (tail && B.carry(consumed, tail))) return -1;
		if (!first) { base += consumed; start = 0; }
		first = false;
		if (src.push(port, 0, &eof)) return -1;
		A.prune(base); A.resolve(false);
		const uint64_t n_text = B.text_bytes();
		if (start > n_text) return al_lift_malformed(fn, base + n_text, AL_LIFT_BAD_CUT);
		AlBaiPiece r;
		if (B.run(start, base, A.tab.data(), A.tab.size(), has_prev, prev_key, &r, rows)) return -1;
		++st.pieces;
		if (r.first_bad != ~0ull && r.bad_off <= r.desc_off) return al_bai_refused(fn, base + r.bad_off, r.bad_code);   // (whichever comes first in the stream)
		if (r.descents) { fprintf(stderr, "ERROR: '%s': not in coordinate order at offset %llu of the inflated stream\n", fn, (unsigned long long)(base + r.desc_off)); return -2; }
		if (r.walk_bad) return al_lift_malformed(fn, base + r.consumed, AL_LIFT_BAD_SIZE);
		if (eof && r.consumed < n_text) return al_lift_malformed(fn, base + r.consumed, AL_LIFT_BAD_CUT);
		consumed = r.consumed; st.records += r.n_rec;
		if (r.n_rec) { has_prev = true; prev_key = r.last_key; }
		A.add(rows, base + n_text);
		if (eof) { A.resolve(true); A.flush(); st.bytes_in = base + n_text; st.read_s += src.read_s; return 0; }
		if (r.n_rec == 0) want *= 2;                                       // no complete record: the next piece is twice as large
	}
}

// ---- the index from the rows and the tables (both backends) ----------------------------------------------------------------------------------------------------------
static inline void al_bai_p32(std::vector<uint8_t> &o, uint32_t v) { for (int i = 0; i < 4; ++i) o.push_back((uint8_t)(v >> (8 * i))); }
static inline void al_bai_p64(std::vector<uint8_t> &o, uint64_t v) { for (int i = 0; i < 8; ++i) o.push_back((uint8_t)(v >> (8 * i))); }
// rows: the runs with refID >= 0 in file order (sorted here).  The file's bytes, CHUNKS / LINEAR INDEX / PSEUDO-BIN of al_dev_bai.h; *chunks: the chunks written
static inline void al_bai_assemble(std::vector<AlBaiRow> &rows, const AlBaiTables &T, std::vector<uint8_t> &out, uint64_t *chunks)
{
	const size_t n_ref = T.ref_len.size();
	std::vector<uint64_t> first(n_ref, 0), last(n_ref, 0); std::vector<uint8_t> any(n_ref, 0);
	for (const AlBaiRow &x : rows) { if (!any[(size_t)x.ref]) { any[(size_t)x.ref] = 1; first[(size_t)x.ref] = x.beg; } last[(size_t)x.ref] = x.end; }
	std::stable_sort(rows.begin(), rows.end(), [](const AlBaiRow &a, const AlBaiRow &b) { return a.ref != b.ref ? a.ref < b.ref : a.bin < b.bin; });
	out.clear(); *chunks = 0;
	out.insert(out.end(), {'B', 'A', 'I', 1}); al_bai_p32(out, (uint32_t)n_ref);
	size_t i = 0;
	for (size_t c = 0; c < n_ref; ++c) {
		const size_t n_bin_at = out.size(); uint32_t n_bin = 0;
		al_bai_p32(out, 0);
		while (i < rows.size() && (size_t)rows[i].ref == c) {
			const uint32_t bin = rows[i].bin; std::vector<AlBaiRow> ch;
			for (; i < rows.size() && (size_t)rows[i].ref == c && rows[i].bin == bin; ++i) {
				if (!ch.empty() && ch.back().end >> 16 >= rows[i].beg >> 16) ch.back().end = rows[i].end; else ch.push_back(rows[i]);
			}
			al_bai_p32(out, bin); al_bai_p32(out, (uint32_t)ch.size());
			for (const AlBaiRow &x : ch) { al_bai_p64(out, x.beg); al_bai_p64(out, x.end); }
			*chunks += ch.size(); ++n_bin;
		}
		if (any[c]) {
			al_bai_p32(out, AL_BAI_PSEUDO); al_bai_p32(out, 2);
			al_bai_p64(out, first[c]); al_bai_p64(out, last[c]); al_bai_p64(out, T.cnt[2 * c]); al_bai_p64(out, T.cnt[2 * c + 1]);
			++n_bin;
		}
		for (int k = 0; k < 4; ++k) out[n_bin_at + k] = (uint8_t)(n_bin >> (8 * k));
		const uint64_t *lin = T.lin.data() + T.lin_off[c]; size_t n_intv = (size_t)(T.lin_off[c + 1] - T.lin_off[c]);
		while (n_intv && lin[n_intv - 1] == ~0ull) --n_intv;
		al_bai_p32(out, (uint32_t)n_intv);
		uint64_t left = 0;
		for (size_t w = 0; w < n_intv; ++w) { if (lin[w] != ~0ull) left = lin[w]; al_bai_p64(out, left); }
	}
	al_bai_p64(out, T.cnt[2 * n_ref]);
}

// ---- the host backend: the twin (al_dev_bai.h) behind the same calls ----------------------------------------------------------------------------------------------
struct AlBaiHostBackend : AlBaiBackend {
	int n_threads; std::vector<uint8_t> txt[2]; int at = 0; std::vector<uint32_t> rec_off; AlBaiTables T;
	double inflate_s = 0, walk_s = 0, key_s = 0;
	typedef AlLiftSource::Timer Timer;
	explicit AlBaiHostBackend(int nt = 1) : n_threads(nt > 1 ? nt : 1) {}
	const char *name() const override { return "host twin"; }
	int set_refs(const uint32_t *len, uint32_t n_ref) override { T.set(len, n_ref); return 0; }
	int begin(size_t cap) override { at ^= 1; txt[at].clear(); txt[at].reserve(cap); return 0; }
	int carry(uint64_t off, uint64_t n) override { const std::vector<uint8_t> &o = txt[at ^ 1]; txt[at].insert(txt[at].end(), o.begin() + (ptrdiff_t)off, o.begin() + (ptrdiff_t)(off + n)); return 0; }
	int append(const uint8_t *p, size_t n) override { txt[at].insert(txt[at].end(), p, p + n); return 0; }
	int append_bgzf(const uint8_t *b, size_t, const AlInfMember *mem, size_t n_mem, uint64_t n_out, size_t *bad, uint32_t *bad_status) override
	{
		Timer tm(inflate_s);
		std::vector<uint8_t> &t = txt[at];
		const size_t a = t.size(); t.resize(a + (size_t)n_out);
		uint8_t *dst = t.data() + a;
		std::atomic<size_t> next{0}; std::vector<uint32_t> status(n_mem, 0);
		auto work = [&]() { for (size_t k; (k = next.fetch_add(1)) < n_mem; ) status[k] = (uint32_t)al_inflate_member_host(b + mem[k].in_off, mem[k].msize, dst + mem[k].out_off); };
		const int nt = (int)std::min<size_t>((size_t)n_threads, n_mem);
		if (nt > 1) { std::vector<std::thread> th; for (int j = 0; j < nt; ++j) th.emplace_back(work); for (auto &x : th) x.join(); } else work();
		for (size_t k = 0; k < n_mem; ++k) if (status[k]) { *bad = k; *bad_status = status[k]; t.resize(a); return 1; }
		return 0;
	}
	uint64_t text_bytes() const override { return txt[at].size(); }
	int run(uint64_t start, uint64_t base, const AlBaiMember *mem, size_t n_mem, bool has_prev, uint64_t prev_key, AlBaiPiece *r, std::vector<AlBaiRow> &rows) override
	{
		*r = AlBaiPiece();
		std::vector<uint8_t> &t = txt[at];
		{ Timer tm(walk_s); al_lift_walk_host(t.data(), t.size(), start, rec_off, &r->consumed, &r->walk_bad); }
		Timer tm(key_s);
		AlBaiStatus s;
		al_bai_piece_host(t.data(), rec_off.data(), rec_off.size(), base, mem, (uint32_t)n_mem, has_prev, prev_key, T, &s, rows);
		r->n_rec = rec_off.size(); r->first_bad = s.first_bad; r->bad_code = s.bad_code; r->descents = s.descents; r->desc_off = s.desc_off; r->last_key = s.last_key;
		if (s.first_bad != ~0ull) r->bad_off = rec_off[(size_t)s.first_bad];
		return 0;
	}
	int tables(AlBaiTables &o) override { o = T; return 0; }
	void *host_buffer(size_t) override { return nullptr; }
	void host_buffer_free(void *) override {}
	void stat(AlBaiRun &st) override { st.inflate_s += inflate_s; st.walk_s += walk_s; st.key_s += key_s; }
};

// ---- one run of the loop over an uncompressed stream, for the taps and tests/csrc/index_main.cpp --------------------------------------------------------------------
// One uncompressed BAM stream (header and records) and its member table through the piece loop of backend B with pieces of `piece` bytes (0: the stream whole).
// bai: the index.  0; -1; -2 refused input; -4 the header is refused.
static inline int al_bai_tap(AlBaiBackend &B, const void *bam, size_t n, const uint64_t *m_file, const uint64_t *m_stream, const uint32_t *m_isize, size_t n_mem, uint64_t file_end, size_t piece,
                             std::vector<uint8_t> &bai, AlBaiRun *run = nullptr)
{
	AlLiftHeader H; size_t used = 0; std::string err;
	if (al_lift_header_parse((const uint8_t *)bam, n, H, &used, err) != 0) { fprintf(stderr, "ERROR: 'input': the header is cut or malformed: %s\n", err.c_str()); return -4; }
	if (B.set_refs(H.len.data(), (uint32_t)H.len.size())) return -1;
	AlBaiAcc A; AlBaiPort port; port.B = &B; port.A = &A;
	AlBaiMemSource src; src.p = (const uint8_t *)bam; src.n = n; src.at = used; src.m_file = m_file; src.m_stream = m_stream; src.m_isize = m_isize; src.n_mem = n_mem; src.file_end = file_end;
	AlBaiRun st;
	const int rc = al_bai_stream(B, src, port, piece ? piece : std::max<size_t>(n, 1), 0, used, "input", A, st);   // (the texts begin behind the header)
	if (rc) return rc;
	AlBaiTables T;
	if (B.tables(T)) return -1;
	al_bai_assemble(A.rows, T, bai, &st.chunks);
	if (run) *run = st;
	return 0;
}

// al_bai.hip: the index of the BGZF file `bam` written to `bai` (nullptr: bam + ".bai") by the twin (host_backend) or by the kernels on `device`; what
// al_index_bam does, and what merge --write-index and lift --sorted --write-index call once their output is closed.  *held: device bytes of the call's account
// at return, *on_device: the kernels ran.  With AL_TIMING=1 it prints the command's line.  0; -1; -2 refused input.
int al_bai_index_file(const char *bam, const char *bai, bool host_backend, int device, int n_threads, size_t piece_bytes, AlBaiRun *run, size_t *held, bool *on_device);

// al_lift.h -- the driver of `lift`: the record stream of one BAM walked in pieces, the function of al_dev_lift.h evaluated by a backend, the kept records and the
// unlifted records' rows handed to the caller.  Host code only, no HIP include: the device backend lives in al_lift.hip, the host backend (the twin) is at the
// end of this file, and tests/csrc/lift_main.cpp runs this loop with the twin under the sanitizers.  Modelled on al_select.h.
//
// A backend holds two texts (slots 0 and 1): inflated BAM bytes.  A piece of the file is appended to a slot's text behind the carry -- the bytes after the last
// complete record of the piece before it, copied from the other slot's text -- then walked, lifted, scanned and gathered: the kept records packed one behind
// the other, and an arena with what the rows of the unlifted records need.  While one slot's gather and copy down run, the other slot takes its carry and its
// piece.  A piece that holds no complete record doubles the next one.  Malformed input ends the walk with error -2 and a message that names the offset of the
// record in the inflated stream.
//
// lift --sorted (set_sorted(true) before the first run()): run() also compacts the kept records to (key, record index) and counts the descents of the compacted
// keys; gather() sorts the pairs when there is a descent (a stable sort) and packs the kept records in that order; sorted_out() gives the keys and the lengths
// of the packed records, what AlRunStore::add_run (al_run_store.h) takes.  The arena is filled as without it.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <unistd.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
#include <vector>
#include "al_dev_lift.h"
#include "al_bgzf_take.h"

struct AlLiftPiece {
	uint64_t n_rec = 0, consumed = 0; uint32_t walk_bad = 0;          // complete records from the start offset on, offset of the first incomplete one, its block_size is out of range
	uint64_t first_bad = ~0ull; uint32_t bad_code = 0; uint64_t bad_off = 0;   // the first record al_lift_record refuses: its number, verdict and offset
	uint64_t kept_bytes = 0, arena_bytes = 0, n_kept = 0, n_unlifted = 0, n_unmapped = 0;
	uint64_t descents = 0;                                            // sorted: positions i of the compacted kept records with key[i] < key[i - 1]
	uint64_t n_packed() const { return n_kept + n_unmapped; }
};
struct AlLiftRun { uint64_t pieces = 0, bytes_in = 0, kept = 0, unlifted = 0, unmapped_kept = 0; double read_s = 0, up_s = 0, inflate_s = 0, walk_s = 0, lift_s = 0, down_s = 0;
	uint64_t in_order = 0, sorted_pieces = 0; double sort_s = 0, sgather_s = 0; };      // lift --sorted: pieces without / with a descent, seconds of the sorts and of the permuted gathers

struct AlLiftBackend {
	virtual ~AlLiftBackend() {}
	virtual const char *name() const = 0;
	virtual int begin(int slot, size_t cap) = 0;                                          // slot's text: empty, room for cap bytes
	virtual int carry(int slot, int from, uint64_t off, uint64_t n) = 0;                  // bytes [off, off + n) of the other slot's text appended
	virtual int append(int slot, const uint8_t *p, size_t n) = 0;                         // host bytes appended
	virtual int append_bgzf(int slot, const uint8_t *bytes, size_t n_in, const AlInfMember *mem, size_t n_mem, uint64_t n_out, size_t *bad, uint32_t *bad_status) = 0;   // whole members inflated to the text's end; 1: *bad has a status
	virtual uint64_t text_bytes(int slot) const = 0;
	virtual int run(int slot, uint64_t start, AlLiftPiece *r) = 0;                        // walk from `start`, lift, scan; returns with the counts
	virtual int gather(int slot, const AlLiftPiece &r, bool packed_down) = 0;             // kept records packed, unlifted records to the arena (may run on); packed_down: the packed bytes come to the host too
	virtual int finish(int slot, const uint8_t **packed, const uint8_t **arena) = 0;      // waits for gather(); the arrays stay until the slot's next gather()
	virtual void *host_buffer(size_t bytes) = 0;                                          // page-locked on the device backend; nullptr: none
	virtual void host_buffer_free(void *p) = 0;
	virtual int fetch_records(int slot, uint32_t *rec_off, uint32_t *verdict, size_t n) = 0;   // of the slot's last run() (the taps)
	virtual void stat(AlLiftRun &) {}                                                     // adds the backend's seconds
	virtual size_t held() const { return 0; }                                             // device bytes of the backend's account
	// lift --sorted
	bool sorted = false;
	void set_sorted(bool on) { sorted = on; }
	virtual int sorted_out(int slot, const uint64_t **keys, const uint32_t **lens) = 0;   // after finish(): key and length of every packed record, in packed order
	virtual int fetch_perm(int slot, uint32_t *perm, size_t n) = 0;                       // after finish(): the record index of every packed record (the taps)
	virtual bool sort_launched(int slot) const = 0;                                       // the slot's last gather() launched a sort (the twin: ran std::stable_sort)
};

struct AlLiftSource {
	virtual ~AlLiftSource() {}
	virtual int read(int slot, size_t want) = 0;                       // 0, or -1 with a message printed
	virtual int push(AlLiftBackend &B, int slot, bool *eof) = 0;       // what read(slot) brought; *eof: the file has ended with it
	virtual size_t pending(int slot) const = 0;                        // upper bound of the text bytes push(slot) will append
	double read_s = 0;
	struct Timer { double &acc; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(); explicit Timer(double &a) : acc(a) {} ~Timer() { acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); } };
};

// BGZF file from a member's file offset on: AlBgzfPieceSource of al_bgzf_take.h over this driver's backend
struct AlLiftBgzfSource : AlBgzfPieceSource<AlLiftBackend, AlLiftSource> { AlLiftBgzfSource() { tag = "lift"; } };

static inline int al_lift_malformed(const char *fn, uint64_t off, uint32_t code)
{
	if (code == AL_LIFT_CG) fprintf(stderr, "ERROR: '%s' holds a CIGAR of more than 65535 operations (CG tag): not supported\n", fn);
	else fprintf(stderr, "ERROR: '%s': malformed BAM record at offset %llu of the inflated stream: %s\n", fn, (unsigned long long)off, al_lift_strerror(code));
	return -2;
}

// The records of one stream through the backend.  The first text's records start at offset `start` of it; base: the stream offset of that text's first byte.
// emit(slot, piece): the slot's gather() has been started; the caller finishes it and writes what it made, pieces in stream order.  0; -1 with a message
// printed; -2 malformed input, its message printed.
template <class Emit> static inline int al_lift_stream(AlLiftBackend &B, AlLiftSource &src, size_t piece, uint64_t start, uint64_t base, const char *fn, bool packed_down, Emit emit, AlLiftRun &st)
{
	if (piece == 0) piece = 1;
	int cur = 0, prev = -1; bool eof = false; size_t want = piece;
	if (src.read(0, want) || B.begin(0, src.pending(0) + 1) || src.push(B, 0, &eof)) return -1;
	AlLiftPiece R[2];
	for (;;) {
		const uint64_t n_text = B.text_bytes(cur);
		if (start > n_text) return al_lift_malformed(fn, base + n_text, AL_LIFT_BAD_CUT);
		if (B.run(cur, start, &R[cur])) return -1;
		const AlLiftPiece &r = R[cur];
		if (r.n_rec == 0) want *= 2;                                       // no complete record: the next piece is twice as large
		if (!eof && src.read(1 - cur, want)) return -1;                    // (the BGZF source only notes the size here: its bytes arrive in push())
		if (r.first_bad != ~0ull) return al_lift_malformed(fn, base + r.bad_off, r.bad_code);
		if (r.walk_bad) return al_lift_malformed(fn, base + r.consumed, AL_LIFT_BAD_SIZE);
		if (eof && r.consumed < n_text) return al_lift_malformed(fn, base + r.consumed, AL_LIFT_BAD_CUT);
		++st.pieces; st.kept += r.n_kept; st.unlifted += r.n_unlifted; st.unmapped_kept += r.n_unmapped;
		if (B.gather(cur, r, packed_down)) return -1;
		if (prev >= 0 && emit(prev, R[prev])) return -1;                 // the piece before: its records leave while this one's are gathered
		if (eof) {
			if (emit(cur, r)) return -1;
			st.bytes_in = base + n_text; st.read_s += src.read_s;
			return 0;
		}
		const uint64_t tail = n_text - r.consumed;
		if (tail + src.pending(1 - cur) + 1 >= (1ull << 31)) { fprintf(stderr, "[ERROR] airlift: lift: '%s': a text of more than 2 GB\n", fn); return -1; }
		if (B.begin(1 - cur, (size_t)tail + src.pending(1 - cur) + 1) || B.carry(1 - cur, cur, r.consumed, tail) || src.push(B, 1 - cur, &eof)) return -1;
		base += r.consumed; start = 0;
		prev = cur; cur = 1 - cur;
	}
}

// The BAM header of a BGZF file: leading members inflated on the host until it is complete.  *file_off / *out_off: file and stream offset of the member
// that holds the first record's first byte, *start that byte's offset in the member.  0; -1 with a message printed.  tag: the command the messages name
// (`merge` reads its inputs' headers with it too).
static inline int lift_read_header(int fd, const char *fn, AlLiftHeader &H, uint64_t *file_off, uint64_t *out_off, uint64_t *start, const char *tag = "lift")
{
	std::vector<uint8_t> in, out; std::vector<uint64_t> m_file, m_out; uint64_t fpos = 0, ipos = 0; bool eof = false;
	for (;;) {
		uint32_t msize = 0, hd = 0; int r = -1;
		if (in.size() - ipos >= 18) r = al_inf_parse_header(in.data() + ipos, in.size() - ipos, &msize, &hd);
		if (r > 0 || (eof && fpos == 0 && in.size() < 28)) { fprintf(stderr, "[ERROR] airlift: %s: '%s' is not a BGZF file (lift reads a BAM by its BGZF members; there is no one-stream reader here)\n", tag, fn); return -1; }
		if (r < 0 || msize > in.size() - ipos) {
			if (eof) { fprintf(stderr, "ERROR: '%s': the file ends inside the BAM header\n", fn); return -2; }
			const size_t at = in.size(); in.resize(at + (1 << 16));
			const ssize_t g = pread(fd, in.data() + at, 1 << 16, (off_t)fpos);
			if (g < 0) { fprintf(stderr, "[ERROR] airlift: %s: reading '%s' failed\n", tag, fn); return -1; }
			in.resize(at + (size_t)g); fpos += (uint64_t)g; if (g == 0) eof = true;
			continue;
		}
		const uint32_t isize = al_inf_le32(in.data() + ipos + msize - 4);
		if (isize > AL_INF_MAX_ISIZE) { fprintf(stderr, "[ERROR] airlift: %s: '%s': no BGZF member at file offset %llu\n", tag, fn, (unsigned long long)ipos); return -1; }
		const size_t at = out.size(); out.resize(at + isize);
		const int stt = al_inflate_member_host(in.data() + ipos, msize, out.data() + at);
		if (stt) { fprintf(stderr, "[ERROR] airlift: %s: '%s': BGZF member at file offset %llu: status %d (%s)\n", tag, fn, (unsigned long long)ipos, stt, al_inf_strerror(stt)); return -1; }
		m_file.push_back(ipos); m_out.push_back(at); ipos += msize;
		size_t used = 0; std::string err;
		const int hr = al_lift_header_parse(out.data(), out.size(), H, &used, err);
		if (hr < 0) { fprintf(stderr, "ERROR: '%s': %s\n", fn, err.c_str()); return -2; }
		if (hr > 0) continue;
		size_t m = m_out.size();
		while (m > 0 && m_out[m - 1] > used) --m;                         // the last member that starts at or before the first record
		if (used == out.size()) { *file_off = ipos; *out_off = out.size(); *start = 0; }
		else { *file_off = m_file[m - 1]; *out_off = m_out[m - 1]; *start = used - m_out[m - 1]; }
		return 0;
	}
}

// ---- the host backend: the twin (al_dev_lift.h) behind the same calls -----------------------------------------------------------------------------------------
struct AlLiftHostBackend : AlLiftBackend {
	AlLiftTab T; int n_threads; std::vector<uint8_t> txt[2], packed[2], arena[2]; std::vector<uint32_t> rec_off[2], verdict[2], keep_len[2], arena_len[2];
	std::vector<uint64_t> key[2], key_s[2]; std::vector<uint32_t> ridx[2], len_s[2];   // sorted: the compacted keys and record indices (ridx: in packed order after gather()), keys and lengths in packed order
	bool did_sort[2] = {false, false};
	double inflate_s = 0, walk_s = 0, lift_s = 0, sort_s = 0, sgather_s = 0;
	typedef AlLiftSource::Timer Timer;
	explicit AlLiftHostBackend(const AlLiftTab &t, int nt = 1) : T(t), n_threads(nt > 1 ? nt : 1) {}
	const char *name() const override { return "host twin"; }
	int begin(int s, size_t cap) override { txt[s].clear(); txt[s].reserve(cap); return 0; }
	int carry(int s, int from, uint64_t off, uint64_t n) override { txt[s].insert(txt[s].end(), txt[from].begin() + (ptrdiff_t)off, txt[from].begin() + (ptrdiff_t)(off + n)); return 0; }
	int append(int s, const uint8_t *p, size_t n) override { txt[s].insert(txt[s].end(), p, p + n); return 0; }
	int append_bgzf(int s, const uint8_t *b, size_t, const AlInfMember *mem, size_t n_mem, uint64_t n_out, size_t *bad, uint32_t *bad_status) override
	{
		Timer tm(inflate_s);
		const size_t at = txt[s].size(); txt[s].resize(at + (size_t)n_out);
		uint8_t *dst = txt[s].data() + at;
		std::atomic<size_t> next{0}; std::vector<uint32_t> status(n_mem, 0);
		auto work = [&]() { for (size_t k; (k = next.fetch_add(1)) < n_mem; ) status[k] = (uint32_t)al_inflate_member_host(b + mem[k].in_off, mem[k].msize, dst + mem[k].out_off); };
		const int nt = (int)std::min<size_t>((size_t)n_threads, n_mem);
		if (nt > 1) { std::vector<std::thread> th; for (int i = 0; i < nt; ++i) th.emplace_back(work); for (auto &x : th) x.join(); } else work();
		for (size_t k = 0; k < n_mem; ++k) if (status[k]) { *bad = k; *bad_status = status[k]; txt[s].resize(at); return 1; }
		return 0;
	}
	uint64_t text_bytes(int s) const override { return txt[s].size(); }
	int run(int s, uint64_t start, AlLiftPiece *r) override
	{
		*r = AlLiftPiece();
		{ Timer tm(walk_s); al_lift_walk_host(txt[s].data(), txt[s].size(), start, rec_off[s], &r->consumed, &r->walk_bad); }
		Timer tm(lift_s);
		const size_t n = rec_off[s].size(); r->n_rec = n;
		verdict[s].resize(n); keep_len[s].resize(n); arena_len[s].resize(n);
		for (size_t k = 0; k < n; ++k) {
			const AlLiftOut o = al_lift_record(T, txt[s].data() + rec_off[s][k]);
			verdict[s][k] = o.verdict; keep_len[s][k] = o.keep_len; arena_len[s][k] = o.arena_len;
			r->kept_bytes += o.keep_len; r->arena_bytes += o.arena_len;
			if (o.verdict == AL_LIFT_KEPT) ++r->n_kept; else if (o.verdict == AL_LIFT_UNLIFTED) ++r->n_unlifted; else if (o.verdict == AL_LIFT_UNMAPPED) ++r->n_unmapped;
			else if (r->first_bad == ~0ull) { r->first_bad = k; r->bad_code = o.verdict; r->bad_off = rec_off[s][k]; }
		}
		if (sorted) {
			key[s].clear(); ridx[s].clear();
			for (size_t k = 0; k < n; ++k) if (verdict[s][k] == AL_LIFT_KEPT || verdict[s][k] == AL_LIFT_UNMAPPED) { key[s].push_back(al_lift_key(txt[s].data() + rec_off[s][k])); ridx[s].push_back((uint32_t)k); }
			for (size_t i = 1; i < key[s].size(); ++i) if (key[s][i] < key[s][i - 1]) ++r->descents;
		}
		return 0;
	}
	int gather(int s, const AlLiftPiece &r, bool) override
	{
		Timer tm(lift_s);
		packed[s].resize((size_t)r.kept_bytes); arena[s].resize((size_t)r.arena_bytes);
		size_t po = 0, ao = 0;
		for (size_t k = 0; k < (size_t)r.n_rec; ++k) {
			const uint8_t *src = txt[s].data() + rec_off[s][k];
			if (verdict[s][k] == AL_LIFT_UNLIFTED) { al_lift_arena_put(src, arena[s].data() + ao, 0, 1); ao += arena_len[s][k]; }
			else if (!sorted && keep_len[s][k]) { memcpy(packed[s].data() + po, src, keep_len[s][k]); po += keep_len[s][k]; }
		}
		if (sorted) {
			const size_t nk = ridx[s].size();
			did_sort[s] = r.descents != 0;
			if (r.descents) {
				Timer ts(sort_s);
				std::vector<uint32_t> perm(nk); for (size_t i = 0; i < nk; ++i) perm[i] = (uint32_t)i;
				std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return key[s][x] < key[s][y]; });
				for (size_t i = 0; i < nk; ++i) perm[i] = ridx[s][perm[i]];
				ridx[s].swap(perm);
			}
			Timer tg(sgather_s);
			key_s[s].resize(nk); len_s[s].resize(nk);
			for (size_t i = 0; i < nk; ++i) {
				const uint32_t k = ridx[s][i]; const uint8_t *src = txt[s].data() + rec_off[s][k];
				key_s[s][i] = al_lift_key(src); len_s[s][i] = keep_len[s][k];
				memcpy(packed[s].data() + po, src, keep_len[s][k]); po += keep_len[s][k];
			}
		}
		return 0;
	}
	int sorted_out(int s, const uint64_t **k, const uint32_t **l) override { *k = key_s[s].data(); *l = len_s[s].data(); return 0; }
	int fetch_perm(int s, uint32_t *perm, size_t n) override { if (n > ridx[s].size()) return -1; if (n) memcpy(perm, ridx[s].data(), n * 4); return 0; }
	bool sort_launched(int s) const override { return did_sort[s]; }
	int finish(int s, const uint8_t **p, const uint8_t **a) override { *p = packed[s].data(); *a = arena[s].data(); return 0; }
	void *host_buffer(size_t) override { return nullptr; }
	void host_buffer_free(void *) override {}
	int fetch_records(int s, uint32_t *ro, uint32_t *v, size_t n) override { if (n) { memcpy(ro, rec_off[s].data(), n * 4); memcpy(v, verdict[s].data(), n * 4); } return 0; }
	void stat(AlLiftRun &st) override { st.inflate_s += inflate_s; st.walk_s += walk_s; st.lift_s += lift_s; st.sort_s += sort_s; st.sgather_s += sgather_s; }
};

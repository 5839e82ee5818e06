// al_select.h -- the driver of --gpu-select (extract-sequence, remap): one FASTQ file walked in pieces, the selection (al_dev_select.h) evaluated by a
// backend, the selected records handed to the caller.  Host code only, no HIP include: the device backend lives in al_select.hip, the host backend
// (the twin) is at the end of this file, and tests/csrc/select_main.cpp runs this loop with the twin under the sanitizers.
//
// A backend holds two texts (slots 0 and 1).  A piece of the file is appended to a slot's text behind the carry -- the bytes after the last complete
// record of the piece before it, copied from the other slot's text -- then indexed, parsed, tested and gathered; only the arena and the descriptors
// come back.  While one slot's gather and copy down run, the other slot takes its carry and its piece: two pieces are in flight.
// Irregular input -- the first record k_fq_parse or al_sel_irregular refuses, or whatever is left behind the last complete record at the end of the
// file -- ends the walk: *handover is that record's offset in the (inflated) stream and the caller gives the rest of the file to the default reader.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <unistd.h>
#include <algorithm>
#include <chrono>
#include <vector>
#include "al_dev_select.h"
#include "al_bgzf_take.h"

struct AlSelPiece {
	uint64_t lines = 0, n_rec = 0, first_bad = ~0ull;      // complete lines, records (lines / 4), first irregular record
	uint64_t n_take = 0, consumed = 0;                    // min(n_rec, first_bad); text offset of record n_take
	uint64_t n_sel = 0, arena_bytes = 0;                  // selected among the n_take, and their bytes
};
struct AlSelStat { uint64_t pieces = 0, bytes_in = 0, tested = 0, selected = 0, handed = 0; double read_s = 0, up_s = 0, kernel_s = 0, down_s = 0; };   // seconds: pread of the pieces; copy up (BGZF: the inflate launch included), kernels, copy down by the backend's events

struct AlSelBackend {
	virtual ~AlSelBackend() {}
	virtual const char *name() const = 0;
	virtual int begin(int slot, size_t cap) = 0;                                          // slot's text: empty, room for cap bytes
	virtual int carry(int slot, int from, uint64_t off, uint64_t n) = 0;                  // bytes [off, off + n) of the other slot's text appended
	virtual int append(int slot, const uint8_t *p, size_t n) = 0;                         // host bytes appended (p stays untouched until the slot's select() has returned)
	virtual int append_bgzf(int slot, const uint8_t *bytes, size_t n_in, const AlInfMember *mem, size_t n_mem, uint64_t n_out, size_t *bad, uint32_t *bad_status) = 0;   // whole members inflated to the text's end; 1: *bad has a status
	virtual int end_text(int slot) = 0;                                                   // the file has ended: a last line without newline gets one
	virtual uint64_t text_bytes(int slot) const = 0;
	virtual int select(int slot, AlSelPiece *r) = 0;                                      // index, parse, test, scan; returns with the counts
	virtual int gather(int slot, const AlSelPiece &r) = 0;                                // the selected of records [0, n_take) to arena + descriptors (may run on)
	virtual int finish(int slot, const uint8_t **arena, const AlSelDesc **desc) = 0;      // waits for gather(); the arrays stay until the slot's next begin()
	virtual void *host_buffer(size_t bytes) = 0;                                          // a buffer append() reads fast from (page-locked on the device backend); nullptr: none
	virtual void host_buffer_free(void *p) = 0;
	virtual int fetch_flags(int slot, uint32_t *dst, size_t n) = 0;                       // flag[0, n) of the slot's last select() (the taps)
	virtual void stat(AlSelStat &) {}                                                     // adds kernel / copy seconds
	virtual size_t held() const { return 0; }                                             // device bytes of the backend's account
};

// where a file's bytes come from: read() brings the next piece to the host (beside the backend's work), push() appends it to a slot's text
struct AlSelSource {
	virtual ~AlSelSource() {}
	virtual int read(int slot, size_t want) = 0;                       // 0, or -1 with a message printed
	virtual int push(AlSelBackend &B, int slot, bool *eof) = 0;        // what read(slot) brought; *eof: the file has ended with it
	virtual size_t pending(int slot) const = 0;                        // upper bound of the text bytes push(slot) will append
	double read_s = 0;                                                 // seconds in pread
	struct Timer { double &acc; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(); explicit Timer(double &a) : acc(a) {} ~Timer() { acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); } };
};

// plain file: pieces by pread into two host buffers
struct AlSelPlainSource : AlSelSource {
	int fd = -1; uint64_t fpos = 0; AlSelBackend *B = nullptr; uint8_t *buf[2] = {nullptr, nullptr}; size_t cap[2] = {0, 0}, n[2] = {0, 0}; bool at_eof[2] = {false, false}, own[2] = {false, false}; const char *fn = "";
	~AlSelPlainSource() { for (int i = 0; i < 2; ++i) drop(i); }
	void drop(int i) { if (buf[i]) { if (own[i]) free(buf[i]); else B->host_buffer_free(buf[i]); } buf[i] = nullptr; cap[i] = 0; }
	int read(int slot, size_t want) override
	{
		if (want > cap[slot]) {
			drop(slot);
			buf[slot] = (uint8_t *)B->host_buffer(want); own[slot] = false;
			if (!buf[slot]) { buf[slot] = (uint8_t *)malloc(want); own[slot] = true; }
			if (!buf[slot]) { fprintf(stderr, "[ERROR] airlift: --gpu-select: no host memory for a piece of %zu bytes\n", want); return -1; }
			cap[slot] = want;
		}
		n[slot] = 0; at_eof[slot] = false;
		Timer tm(read_s);
		while (n[slot] < want) {
			const ssize_t g = pread(fd, buf[slot] + n[slot], want - n[slot], (off_t)fpos);
			if (g < 0) { fprintf(stderr, "[ERROR] airlift: --gpu-select: reading '%s' failed\n", fn); return -1; }
			if (g == 0) { at_eof[slot] = true; break; }
			n[slot] += (size_t)g; fpos += (uint64_t)g;
		}
		return 0;
	}
	int push(AlSelBackend &Bk, int slot, bool *eof) override { *eof = at_eof[slot]; return n[slot] ? Bk.append(slot, buf[slot], n[slot]) : 0; }
	size_t pending(int slot) const override { return n[slot]; }
};

// BGZF file (--gpu-inflate as well): AlBgzfPieceSource of al_bgzf_take.h over this driver's backend
struct AlSelBgzfSource : AlBgzfPieceSource<AlSelBackend, AlSelSource> { AlSelBgzfSource() { tag = "--gpu-select"; } };

// One file through the backend.  emit(arena, desc, n): the selected records of one piece, in file order.  *handover: ~0, or the stream offset the default
// reader continues at.  0, or -1 with a message printed.
template <class Emit> static inline int al_select_file(AlSelBackend &B, AlSelSource &src, size_t piece, Emit emit, uint64_t *handover, AlSelStat &st)
{
	*handover = ~0ull;
	if (piece == 0) piece = 1;
	int cur = 0, prev = -1; uint64_t base = 0; bool eof = false; size_t want = piece;
	if (src.read(0, want) || B.begin(0, src.pending(0) + 1) || src.push(B, 0, &eof)) return -1;
	if (eof && B.end_text(0)) return -1;
	AlSelPiece R[2];
	for (;;) {
		const uint64_t n_text = B.text_bytes(cur);
		if (!eof && src.read(1 - cur, want)) return -1;                    // the next piece comes to the host beside this one's copy up and index
		if (B.select(cur, &R[cur])) return -1;
		const AlSelPiece &r = R[cur];
		++st.pieces; st.tested += r.n_take; st.selected += r.n_sel;
		const bool irregular = r.first_bad < r.n_rec || (eof && r.consumed < n_text);
		if (B.gather(cur, r)) return -1;
		if (prev >= 0) {                                                   // the piece before: its records leave while this one's are gathered
			const uint8_t *arena = nullptr; const AlSelDesc *desc = nullptr;
			if (B.finish(prev, &arena, &desc) || emit(arena, desc, (size_t)R[prev].n_sel)) return -1;
		}
		if (irregular || eof) {
			const uint8_t *arena = nullptr; const AlSelDesc *desc = nullptr;
			if (B.finish(cur, &arena, &desc) || emit(arena, desc, (size_t)r.n_sel)) return -1;
			if (irregular) *handover = base + r.consumed;
			st.bytes_in = base + n_text; st.read_s += src.read_s;
			return 0;
		}
		const uint64_t tail = n_text - r.consumed;
		if (tail + src.pending(1 - cur) + 1 >= (1ull << 31)) { fprintf(stderr, "[ERROR] airlift: --gpu-select: a record of more than 2 GB\n"); return -1; }
		if (B.begin(1 - cur, (size_t)tail + src.pending(1 - cur) + 1) || B.carry(1 - cur, cur, r.consumed, tail) || src.push(B, 1 - cur, &eof)) return -1;
		if (eof && B.end_text(1 - cur)) return -1;
		if (r.n_take == 0) want *= 2;                                      // a record longer than the window: the window grows
		base += r.consumed;
		prev = cur; cur = 1 - cur;
	}
}

// ---- the host backend: the twin (al_dev_select.h) behind the same calls ---------------------------------------------------------------------------------------
struct AlSelHostBackend : AlSelBackend {
	AlSelTable T; std::vector<uint8_t> txt[2], arena[2]; std::vector<AlSelDesc> desc[2]; std::vector<uint32_t> ls, flag[2], bytes; std::vector<AlFqRec> rec[2];
	explicit AlSelHostBackend(const AlSelTable &t) : T(t) {}
	const char *name() const override { return "host twin"; }
	int begin(int s, size_t cap) override { txt[s].clear(); txt[s].reserve(cap); return 0; }
	int carry(int s, int from, uint64_t off, uint64_t n) override { txt[s].insert(txt[s].end(), txt[from].begin() + (ptrdiff_t)off, txt[from].begin() + (ptrdiff_t)(off + n)); return 0; }
	int append(int s, const uint8_t *p, size_t n) override { txt[s].insert(txt[s].end(), p, p + n); return 0; }
	int append_bgzf(int s, const uint8_t *b, size_t, const AlInfMember *mem, size_t n_mem, uint64_t n_out, size_t *bad, uint32_t *bad_status) override
	{
		const size_t at = txt[s].size(); txt[s].resize(at + (size_t)n_out);
		for (size_t k = 0; k < n_mem; ++k) {
			const int stt = al_inflate_member_host(b + mem[k].in_off, mem[k].msize, txt[s].data() + at + mem[k].out_off);
			if (stt) { *bad = k; *bad_status = (uint32_t)stt; txt[s].resize(at); return 1; }
		}
		return 0;
	}
	int end_text(int s) override { if (!txt[s].empty() && txt[s].back() != '\n') txt[s].push_back('\n'); return 0; }
	uint64_t text_bytes(int s) const override { return txt[s].size(); }
	int select(int s, AlSelPiece *r) override
	{
		const uint8_t *t = txt[s].data();
		al_sel_lines_host(t, txt[s].size(), ls);
		r->lines = ls.size() - 1; r->n_rec = r->lines / 4; r->first_bad = ~0ull;
		const uint32_t n = (uint32_t)r->n_rec;
		rec[s].resize(n); flag[s].resize(n); bytes.resize(n);
		for (uint32_t k = 0; k < n; ++k) if (!al_sel_parse_host(t, ls.data(), k, rec[s][k]) && r->first_bad == ~0ull) r->first_bad = k;
		r->first_bad = std::min(r->first_bad, al_sel_select_host(t, rec[s].data(), n, T, flag[s].data(), bytes.data()));
		r->n_take = std::min(r->n_rec, r->first_bad); r->consumed = ls[4 * r->n_take];
		r->n_sel = 0; r->arena_bytes = 0;
		for (uint64_t k = 0; k < r->n_take; ++k) { r->n_sel += flag[s][k]; r->arena_bytes += bytes[k]; }
		return 0;
	}
	int gather(int s, const AlSelPiece &r) override
	{
		arena[s].resize((size_t)r.arena_bytes); desc[s].resize((size_t)r.n_sel);
		al_sel_gather_host(txt[s].data(), rec[s].data(), (uint32_t)r.n_take, flag[s].data(), desc[s].data(), arena[s].data());
		return 0;
	}
	int finish(int s, const uint8_t **a, const AlSelDesc **d) override { *a = arena[s].data(); *d = desc[s].data(); return 0; }
	int fetch_flags(int s, uint32_t *dst, size_t n) override { if (n) memcpy(dst, flag[s].data(), n * 4); return 0; }
	void *host_buffer(size_t) override { return nullptr; }
	void host_buffer_free(void *) override {}
};

// ---- the product's entry (al_select.hip) -------------------------------------------------------------------------------------------------------------------------
#include <functional>
typedef std::function<int(const uint8_t *arena, const AlSelDesc *desc, size_t n)> AlSelEmit;
// File fn against the names N.  host_backend: the twin is asked for (AL_EXTRACT_SELECT_HOST); otherwise `device` (-1: the default device) runs the kernels, and
// the twin takes over, with one notice, where there is no usable device or its memory is refused.  gpu_inflate: a BGZF file is inflated into the text.
// 0: done, *handover = ~0 or the stream offset the default reader continues at; 1: the file is not for the selector (another gzip file, "-": one
// notice is printed) and the default reader takes all of it; -1: an error, its message printed.  Every device range is released before it returns
// (*held: the bytes its account still shows, 0).
int al_select_subseq(const char *fn, const AlSelNames &N, bool host_backend, bool gpu_inflate, int device, size_t piece_bytes, const AlSelEmit &emit,
                     uint64_t *handover, AlSelStat *st, const char **backend, size_t *held);

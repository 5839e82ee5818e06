// al_merge.h -- the driver of `merge`: K coordinate-sorted BAM streams walked in pieces, the function of al_dev_merge.h evaluated by a backend, the merged records
// handed to the caller round by round.  Host code only, no HIP include: the device backend lives in al_merge.hip, the host backend (the twin) is at the end of
// this file, and tests/csrc/merge_main.cpp runs this loop with the twin under the sanitizers.  Modelled on al_lift.h.
//
// A backend holds, per input, a window: a text of inflated BAM bytes (two buffers that take turns, so that the carry -- the bytes after the last complete record
// -- is copied from the one to the other), the offsets, keys and lengths of its complete records.  A window is refilled only when the rounds have emitted all its
// records.  A round (THE STREAMING RULE in al_dev_merge.h): bounds() says how many records each input emits, merge() merges those runs -- (key, tag) pairs, a
// stable merge in which the earlier input wins ties -- and packs the records in that order into one of two packed buffers; while the caller writes one round's
// bytes, the next round's kernels run.  Malformed and unsorted input ends the loop with -2 and a message that names the offset in the inflated stream.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <unistd.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
#include <vector>
#include "al_dev_merge.h"
#include "al_lift.h"               // lift_read_header, al_lift_malformed; al_bgzf_take.h

struct AlMergePiece {
	uint64_t n_rec = 0, consumed = 0; uint32_t walk_bad = 0;          // complete records from the start offset on, offset of the first incomplete one, its block_size is out of range
	uint64_t first_bad = ~0ull, bad_off = 0;                          // the first record with a refID beyond the input's list: its number and offset
	uint64_t descents = 0, desc_off = ~0ull, last_key = 0;            // records below their predecessor, the smallest offset of one; the key of the last record
};
struct AlMergeRound { uint64_t n = 0, bytes = 0; };                   // a round's records and their bytes
struct AlMergeRun { uint64_t rounds = 0, refills = 0, bytes_in = 0, records = 0, recs[AL_MERGE_MAX_IN] = {}; double read_s = 0, up_s = 0, inflate_s = 0, walk_s = 0, key_s = 0, merge_s = 0, gather_s = 0, down_s = 0; };

struct AlMergeBackend {
	virtual ~AlMergeBackend() {}
	virtual const char *name() const = 0;
	virtual int set_map(int i, const int32_t *map, uint32_t n_ref) = 0;                   // input i's table old refID -> new refID, before its first run()
	virtual int begin(int i, size_t cap) = 0;                                             // input i's other text: empty, room for cap bytes; it is the current one from here on
	virtual int carry(int i, uint64_t off, uint64_t n) = 0;                               // bytes [off, off + n) of the text that was current before begin(), appended
	virtual int append(int i, const uint8_t *p, size_t n) = 0;                            // host bytes appended
	virtual int append_bgzf(int i, const uint8_t *bytes, size_t n_in, const AlInfMember *mem, size_t n_mem, uint64_t n_out, size_t *bad, uint32_t *bad_status) = 0;   // whole members inflated to the text's end; 1: *bad has a status
	virtual uint64_t text_bytes(int i) const = 0;
	virtual int run(int i, uint64_t start, bool has_prev, uint64_t prev_key, AlMergePiece *r) = 0;   // walk from `start`, keys; prev_key: the last key of the input's window before
	virtual int bounds(const uint32_t *cur, const uint32_t *n, const uint8_t *eof, int k, uint32_t *cnt, uint64_t *total) = 0;   // the records each input emits in this round
	virtual int merge(int slot, const uint32_t *cur, const uint32_t *cnt, int k, bool packed_down, AlMergeRound *r) = 0;   // the runs merged, the records packed in that order (may run on); packed_down: the bytes come to the host too
	virtual int finish(int slot, const uint8_t **packed) = 0;                             // waits for merge(); the bytes stay until the slot's next merge()
	virtual int fetch_merged(int slot, uint32_t *tags, uint64_t *keys, size_t n) = 0;     // after finish(): tag and key of every packed record (the taps)
	virtual void *host_buffer(size_t bytes) = 0;                                          // page-locked on the device backend; nullptr: none
	virtual void host_buffer_free(void *p) = 0;
	virtual void stat(AlMergeRun &) {}                                                    // adds the backend's seconds
	virtual size_t held() const { return 0; }                                             // device bytes of the backend's account
};

// what AlBgzfPieceSource takes for a backend: input i of the merge's backend
struct AlMergePort {
	AlMergeBackend *B = nullptr; int i = 0;
	int append(int, const uint8_t *p, size_t n) { return B->append(i, p, n); }
	int append_bgzf(int, const uint8_t *bytes, size_t n_in, const AlInfMember *mem, size_t n_mem, uint64_t n_out, size_t *bad, uint32_t *bad_status) { return B->append_bgzf(i, bytes, n_in, mem, n_mem, n_out, bad, bad_status); }
	void *host_buffer(size_t n) { return B->host_buffer(n); }
	void host_buffer_free(void *p) { B->host_buffer_free(p); }
};
struct AlMergeSource {
	virtual ~AlMergeSource() {}
	virtual int read(int slot, size_t want) = 0;                       // 0, or -1 with a message printed (slot is always 0 here)
	virtual int push(AlMergePort &B, int slot, bool *eof) = 0;         // what read() brought; *eof: the stream has ended with it
	virtual size_t pending(int slot) const = 0;                        // upper bound of the text bytes push() will append
	double read_s = 0;
	typedef AlLiftSource::Timer Timer;
};
// BGZF file from a member's file offset on
struct AlMergeBgzfSource : AlBgzfPieceSource<AlMergePort, AlMergeSource> { AlMergeBgzfSource() { tag = "merge"; } };
// an uncompressed stream in memory (the taps, tests/csrc/merge_main.cpp)
struct AlMergeMemSource : AlMergeSource {
	const uint8_t *p = nullptr; size_t n = 0, at = 0, want = 0;
	int read(int, size_t w) override { want = w; return 0; }
	size_t pending(int) const override { return std::min(want, n - at); }
	int push(AlMergePort &B, int, bool *eof) override { const size_t m = std::min(want, n - at); if (B.append(0, p + at, m)) return -1; at += m; *eof = at == n; return 0; }
};

struct AlMergeIn {
	AlMergeSource *src = nullptr; AlMergePort port; const char *fn = "";
	uint64_t start = 0, base = 0;                                     // where the first text's first record starts; the stream offset of the current text's first byte
	size_t want = 0; uint32_t cur = 0, n = 0; bool eof = false, first = true, has_prev = false; uint64_t prev_key = 0, consumed = 0;
};

// input i's window refilled until it holds a record or the input has ended.  0; -1 with a message printed; -2 malformed or unsorted input, its message printed.
static inline int al_merge_fill(AlMergeBackend &B, AlMergeIn &I, int i, AlMergeRun &st)
{
	for (;;) {
		const uint64_t tail = I.first ? 0 : B.text_bytes(i) - I.consumed;
		if (I.src->read(0, I.want)) return -1;
		const size_t pend = I.src->pending(0);
		if (tail + pend + 1 >= (1ull << 31)) { fprintf(stderr, "[ERROR] airlift: merge: '%s': a text of more than 2 GB\n", I.fn); return -1; }
		if (B.begin(i, (size_t)tail + pend + 1) || (tail && B.carry(i, I.consumed, tail))) return -1;
		if (!I.first) { I.base += I.consumed; I.start = 0; }
		I.first = false;
		if (I.src->push(I.port, 0, &I.eof)) return -1;
		const uint64_t n_text = B.text_bytes(i);
		if (I.start > n_text) return al_lift_malformed(I.fn, I.base + n_text, AL_LIFT_BAD_CUT);
		AlMergePiece r;
		if (B.run(i, I.start, I.has_prev, I.prev_key, &r)) return -1;
		++st.refills;
		if (r.first_bad != ~0ull && r.bad_off <= r.desc_off) return al_lift_malformed(I.fn, I.base + r.bad_off, AL_LIFT_BAD_REF);   // (whichever comes first in the stream)
		if (r.descents) { fprintf(stderr, "ERROR: '%s': not in coordinate order at offset %llu of the inflated stream\n", I.fn, (unsigned long long)(I.base + r.desc_off)); return -2; }
		if (r.walk_bad) return al_lift_malformed(I.fn, I.base + r.consumed, AL_LIFT_BAD_SIZE);
		if (I.eof && r.consumed < n_text) return al_lift_malformed(I.fn, I.base + r.consumed, AL_LIFT_BAD_CUT);
		if (r.n_rec >= (1ull << AL_MERGE_TAG_BITS)) { fprintf(stderr, "[ERROR] airlift: merge: '%s': a window of 2^28 records or more; use a smaller --piece\n", I.fn); return -1; }
		I.consumed = r.consumed; I.cur = 0; I.n = (uint32_t)r.n_rec;
		if (r.n_rec) { I.has_prev = true; I.prev_key = r.last_key; }
		st.recs[i] += r.n_rec;
		if (I.eof) st.bytes_in += I.base + n_text;
		if (r.n_rec == 0 && !I.eof) { I.want *= 2; continue; }              // no complete record: the next piece is twice as large
		return 0;
	}
}

// The k streams of `in` through the backend.  emit(slot, round): the slot's merge() has been started; the caller finishes it and writes what it made, rounds in
// order.  0; -1 with a message printed; -2 malformed or unsorted input, its message printed.
template <class Emit> static inline int al_merge_stream(AlMergeBackend &B, AlMergeIn *in, int k, size_t piece, bool packed_down, Emit emit, AlMergeRun &st)
{
	if (piece == 0) piece = 1;
	for (int i = 0; i < k; ++i) { in[i].want = piece; in[i].port.B = &B; in[i].port.i = i; if (const int e = al_merge_fill(B, in[i], i, st)) return e; }
	int slot = 0, prev = -1; AlMergeRound R[2];
	for (;;) {
		uint32_t cur[AL_MERGE_MAX_IN], n[AL_MERGE_MAX_IN], cnt[AL_MERGE_MAX_IN]; uint8_t eof[AL_MERGE_MAX_IN]; uint64_t total = 0; bool left = false;
		for (int i = 0; i < k; ++i) { cur[i] = in[i].cur; n[i] = in[i].n; eof[i] = in[i].eof; if (cur[i] < n[i]) left = true; }
		if (!left) break;
		if (B.bounds(cur, n, eof, k, cnt, &total)) return -1;
		if (total == 0) { fprintf(stderr, "[airlift] merge: a round without a record\n"); return -1; }
		if (B.merge(slot, cur, cnt, k, packed_down, &R[slot])) return -1;
		++st.rounds; st.records += total;
		for (int i = 0; i < k; ++i) in[i].cur += cnt[i];
		if (prev >= 0 && emit(prev, R[prev])) return -1;                 // the round before: its records leave while this one's are merged
		prev = slot; slot = 1 - slot;
		for (int i = 0; i < k; ++i) if (in[i].cur == in[i].n && !in[i].eof) if (const int e = al_merge_fill(B, in[i], i, st)) return e;
	}
	if (prev >= 0 && emit(prev, R[prev])) return -1;
	for (int i = 0; i < k; ++i) st.read_s += in[i].src->read_s;
	return 0;
}

// ---- the host backend: the twin (al_dev_merge.h) behind the same calls --------------------------------------------------------------------------------------------
struct AlMergeHostBackend : AlMergeBackend {
	int n_threads; std::vector<uint8_t> txt[AL_MERGE_MAX_IN][2], packed[2]; int at[AL_MERGE_MAX_IN] = {};
	std::vector<uint32_t> rec_off[AL_MERGE_MAX_IN], rlen[AL_MERGE_MAX_IN], tags[2]; std::vector<uint64_t> key[AL_MERGE_MAX_IN], mkey[2];
	const int32_t *map[AL_MERGE_MAX_IN] = {}; uint32_t n_ref[AL_MERGE_MAX_IN] = {};
	double inflate_s = 0, walk_s = 0, key_s = 0, merge_s = 0, gather_s = 0;
	typedef AlLiftSource::Timer Timer;
	explicit AlMergeHostBackend(int nt = 1) : n_threads(nt > 1 ? nt : 1) {}
	const char *name() const override { return "host twin"; }
	int set_map(int i, const int32_t *m, uint32_t nr) override { map[i] = m; n_ref[i] = nr; return 0; }
	std::vector<uint8_t> &text(int i) { return txt[i][at[i]]; }
	int begin(int i, size_t cap) override { at[i] ^= 1; text(i).clear(); text(i).reserve(cap); return 0; }
	int carry(int i, uint64_t off, uint64_t n) override { const std::vector<uint8_t> &o = txt[i][at[i] ^ 1]; text(i).insert(text(i).end(), o.begin() + (ptrdiff_t)off, o.begin() + (ptrdiff_t)(off + n)); return 0; }
	int append(int i, const uint8_t *p, size_t n) override { text(i).insert(text(i).end(), p, p + n); return 0; }
	int append_bgzf(int i, const uint8_t *b, size_t, const AlInfMember *mem, size_t n_mem, uint64_t n_out, size_t *bad, uint32_t *bad_status) override
	{
		Timer tm(inflate_s);
		std::vector<uint8_t> &t = text(i);
		const size_t a = t.size(); t.resize(a + (size_t)n_out);
		uint8_t *dst = t.data() + a;
		std::atomic<size_t> next{0}; std::vector<uint32_t> status(n_mem, 0);
		auto work = [&]() { for (size_t k; (k = next.fetch_add(1)) < n_mem; ) status[k] = (uint32_t)al_inflate_member_host(b + mem[k].in_off, mem[k].msize, dst + mem[k].out_off); };
		const int nt = (int)std::min<size_t>((size_t)n_threads, n_mem);
		if (nt > 1) { std::vector<std::thread> th; for (int j = 0; j < nt; ++j) th.emplace_back(work); for (auto &x : th) x.join(); } else work();
		for (size_t k = 0; k < n_mem; ++k) if (status[k]) { *bad = k; *bad_status = status[k]; t.resize(a); return 1; }
		return 0;
	}
	uint64_t text_bytes(int i) const override { return txt[i][at[i]].size(); }
	int run(int i, uint64_t start, bool has_prev, uint64_t prev_key, AlMergePiece *r) override
	{
		*r = AlMergePiece();
		std::vector<uint8_t> &t = text(i);
		{ Timer tm(walk_s); al_lift_walk_host(t.data(), t.size(), start, rec_off[i], &r->consumed, &r->walk_bad); }
		Timer tm(key_s);
		const size_t n = rec_off[i].size(); r->n_rec = n;
		key[i].resize(n + 1); rlen[i].resize(n + 1);
		al_merge_keys_host(t.data(), rec_off[i].data(), n, map[i], n_ref[i], has_prev, prev_key, key[i].data(), rlen[i].data(), &r->first_bad, &r->descents, &r->desc_off);
		if (r->first_bad != ~0ull) r->bad_off = rec_off[i][(size_t)r->first_bad];
		if (n) r->last_key = key[i][n - 1];
		return 0;
	}
	int bounds(const uint32_t *cur, const uint32_t *n, const uint8_t *eof, int k, uint32_t *cnt, uint64_t *total) override
	{
		AlMergeWins W; W.k = (uint32_t)k; *total = 0;
		for (int i = 0; i < k; ++i) W.w[i] = AlMergeWin{key[i].data(), cur[i], n[i], eof[i]};
		for (int i = 0; i < k; ++i) { cnt[i] = al_merge_emit_count(W, (uint32_t)i); *total += cnt[i]; }
		return 0;
	}
	// a plain stable k-way merge: the smallest head, the earliest input among equal ones
	int merge(int s, const uint32_t *cur, const uint32_t *cnt, int k, bool, AlMergeRound *r) override
	{
		uint32_t c[AL_MERGE_MAX_IN], e[AL_MERGE_MAX_IN]; size_t total = 0;
		for (int i = 0; i < k; ++i) { c[i] = cur[i]; e[i] = cur[i] + cnt[i]; total += cnt[i]; }
		tags[s].clear(); mkey[s].clear(); tags[s].reserve(total); mkey[s].reserve(total);
		{
			Timer tm(merge_s);
			for (size_t o = 0; o < total; ++o) {
				int best = -1;
				for (int i = 0; i < k; ++i) if (c[i] < e[i] && (best < 0 || key[i][c[i]] < key[best][c[best]])) best = i;
				tags[s].push_back((uint32_t)best << AL_MERGE_TAG_BITS | c[best]); mkey[s].push_back(key[best][c[best]]); ++c[best];
			}
		}
		Timer tm(gather_s);
		size_t bytes = 0;
		for (uint32_t t : tags[s]) bytes += rlen[t >> AL_MERGE_TAG_BITS][t & AL_MERGE_TAG_MASK];
		packed[s].resize(bytes); size_t po = 0;
		for (uint32_t t : tags[s]) { const int i = (int)(t >> AL_MERGE_TAG_BITS); const uint32_t x = t & AL_MERGE_TAG_MASK; memcpy(packed[s].data() + po, text(i).data() + rec_off[i][x], rlen[i][x]); po += rlen[i][x]; }
		r->n = total; r->bytes = bytes;
		return 0;
	}
	int finish(int s, const uint8_t **p) override { *p = packed[s].data(); return 0; }
	int fetch_merged(int s, uint32_t *t, uint64_t *k, size_t n) override { if (n > tags[s].size()) return -1; if (n) { memcpy(t, tags[s].data(), n * 4); memcpy(k, mkey[s].data(), n * 8); } return 0; }
	void *host_buffer(size_t) override { return nullptr; }
	void host_buffer_free(void *) override {}
	void stat(AlMergeRun &st) override { st.inflate_s += inflate_s; st.walk_s += walk_s; st.key_s += key_s; st.merge_s += merge_s; st.gather_s += gather_s; }
};

// ---- one run of the loop over uncompressed streams, for the taps and tests/csrc/merge_main.cpp -------------------------------------------------------------------
// k uncompressed BAM streams (header and records) through the round loop of backend B with pieces of `piece` bytes (0: each stream whole, so that there is one
// round with every input at eof).  tags / keys[0, *n_out) and packed[0, *packed_n): every round's merged records one behind the other (room for rec_cap records
// and packed_cap bytes; a tag's record index counts within its round's window).  0; -1; -2 malformed or unsorted; -3 room; -4 a header is refused.
static inline int al_merge_tap(AlMergeBackend &B, const void *const *bam, const size_t *n, int k, size_t piece, uint32_t *tags, uint64_t *keys, size_t rec_cap, size_t *n_out,
                               void *packed, size_t packed_cap, size_t *packed_n, uint64_t *rounds)
{
	*n_out = 0; *packed_n = 0; if (rounds) *rounds = 0;
	if (k < 2 || k > AL_MERGE_MAX_IN) return -4;
	std::vector<AlLiftHeader> H((size_t)k); std::vector<std::string> fn; std::vector<size_t> start((size_t)k); std::vector<std::string> names((size_t)k); std::string err;
	for (int i = 0; i < k; ++i) {
		names[(size_t)i] = "input " + std::to_string(i + 1); fn.push_back(names[(size_t)i]);
		if (al_lift_header_parse((const uint8_t *)bam[i], n[i], H[(size_t)i], &start[(size_t)i], err) != 0) { fprintf(stderr, "ERROR: '%s': the header is cut or malformed: %s\n", fn.back().c_str(), err.c_str()); return -4; }
	}
	AlMergeHeaders M;
	if (al_merge_headers(H, fn, M, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return -4; }
	std::vector<AlMergeMemSource> src((size_t)k); AlMergeIn in[AL_MERGE_MAX_IN]; size_t whole = 1;
	for (int i = 0; i < k; ++i) {
		if (B.set_map(i, M.map[(size_t)i].data(), (uint32_t)H[(size_t)i].name.size())) return -1;
		src[(size_t)i].p = (const uint8_t *)bam[i]; src[(size_t)i].n = n[i]; src[(size_t)i].at = start[(size_t)i]; in[i].src = &src[(size_t)i]; in[i].fn = names[(size_t)i].c_str(); in[i].start = 0; in[i].base = start[(size_t)i];   // (the texts begin behind the header)
		whole = std::max(whole, n[i]);
	}
	AlMergeRun st; bool room = true;
	const int rc = al_merge_stream(B, in, k, piece ? piece : whole, true, [&](int slot, const AlMergeRound &r) -> int {
		const uint8_t *p = nullptr;
		if (B.finish(slot, &p)) return -1;
		if (room && *n_out + r.n <= rec_cap && *packed_n + r.bytes <= packed_cap) {
			if (B.fetch_merged(slot, tags + *n_out, keys + *n_out, (size_t)r.n)) return -1;
			if (r.bytes) memcpy((uint8_t *)packed + *packed_n, p, (size_t)r.bytes);
		} else room = false;
		*n_out += (size_t)r.n; *packed_n += (size_t)r.bytes;
		return 0;
	}, st);
	if (rounds) *rounds = st.rounds;
	return rc ? rc : room ? 0 : -3;
}

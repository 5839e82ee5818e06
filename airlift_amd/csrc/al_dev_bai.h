// al_dev_bai.h -- `bam-index`: the BAI of a coordinate-sorted BAM (run_pipeline.sh:9, :95 and :119, samtools index) as ONE function of the BAM's records and of
// the table of the BGZF members they lie in, written once for both sides: the pieces below are compiled for the device (k_bai_key, k_bai_heads, k_bai_rows,
// k_bai_lin: al_bai.hip) and for the CPU (the twin at the end of this file).  The twin is what the kernels are tested against, what `bam-index --host` runs and
// what tests/csrc/index_main.cpp runs under the sanitizers.  tests/index_cases.py states the same rules in Python.  Byte parity with samtools index is NOT claimed:
// htslib's order of the bins and its folding of small bins into their parents are not part of the format.  The index is defined by the rules below; that it is
// right is shown by the query procedure of the SAM specification (section 5.3), which must find exactly the records a scan of the file finds.
//
// INPUT.  A BGZF BAM in coordinate order by al_lift_key (al_dev_lift.h), as `merge` requires it: a record whose key is below the key of the one before it -- across
// a piece boundary too -- is refused with merge's message.  Refused with lift's messages: what the walk refuses, a name and CIGAR that do not fit block_size (the
// CIGAR is read here), a refID at or beyond the header's n_ref.
//
// INTERVAL of a record with refID >= 0 (al_bai_record).  beg = max(pos, 0); end = beg + reflen, reflen the sum of the CIGAR operations M, D, N, = and X; with flag 4
// set or reflen 0, end = beg + 1.  bin = reg2bin(beg, end): the record's own bin field is not trusted.  Refused: end > 2^29 (the BAI format ends there; CSI is not
// built), and, for a record with flag 4 clear, end > the contig's LN (the linear index has ceil(LN / 2^14) windows per contig and no window beyond them).
//
// VIRTUAL OFFSETS (al_bai_voff).  For stream offset s: the member with out_off <= s < out_off + isize -- a member of isize 0 never matches -- gives
// file_off << 16 | (s - out_off).  So a record that ends exactly at a member's end has the end offset (next non-empty member, 0), and the end of the file's last
// record, when no non-empty member follows, is (the file offset behind the last non-empty member, 0).  A piece's table need not hold the member behind its text:
// the end of the piece's last record is then AL_BAI_OPEN, and the driver (al_bai.h) sets it once the next piece's members, or the end of the file, are known.
//
// CHUNKS.  A maximal run of consecutive records with the same (refID, bin) is one chunk, from the offset of its first record's start to the offset of its last
// record's end.  A bin's chunks stay in file order; a chunk and the next one of the same bin are joined when a.end >> 16 >= b.beg >> 16.  Bins are not folded.
//
// LINEAR INDEX of a contig.  n_intv = ((the largest end - 1 over its records with flag 4 clear) >> 14) + 1, 0 without such a record; ioffset[w] = the smallest
// start offset of such a record whose [beg, end) touches window w; a window no record touches takes its left neighbour's value, leading ones 0.
//
// PSEUDO-BIN 37450 of every contig with a record: chunk 0 = (start offset of the contig's first record, end offset of its last), chunk 1 = (records with flag 4
// clear, records with flag 4 set).  A contig without a record: n_bin = 0, n_intv = 0.  n_no_coor, the records with refID < 0, is always written.  Contigs in
// header order; within a contig the bins ascending, 37450 last.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "al_dev_lift.h"

#define AL_BAI_MAX_END (1ll << 29)
#define AL_BAI_MAX_WIN (1u << 15)                   // windows of a contig: 2^29 >> 14
#define AL_BAI_PSEUDO 37450u
#define AL_BAI_OPEN (~0ull)
enum { AL_BAI_BAD_BIG = 16, AL_BAI_BAD_LN = 17 };   // beside the AL_LIFT_BAD_* codes

struct AlBaiMember { uint64_t s_off, file_off; uint32_t isize, msize; };            // a BGZF member: where its first byte lies in the inflated stream and in the file
struct alignas(16) AlBaiRec { int32_t ref; uint32_t bin, win, pad; uint64_t vbeg, vend; };   // win: first window | last window << 16 | (flag 4 clear) << 31; ref -1: unplaced, or refused
struct AlBaiRow { int32_t ref; uint32_t bin; uint64_t beg, end; };                  // a run of records of one (refID, bin)

AL_DHD uint32_t al_bai_n_win(uint32_t ln) { const uint64_t w = ((uint64_t)ln + 16383) >> 14; return w < AL_BAI_MAX_WIN ? (uint32_t)w : AL_BAI_MAX_WIN; }
// the virtual offset of stream offset s in the table m[0, n) (members in stream order), AL_BAI_OPEN when no member of the table holds s
AL_DHD uint64_t al_bai_voff(const AlBaiMember *m, uint32_t n, uint64_t s)
{
	uint32_t lo = 0, hi = n;                                        // the first member that ends beyond s
	while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (m[mid].s_off + m[mid].isize <= s) lo = mid + 1; else hi = mid; }
	if (lo == n || m[lo].s_off > s) return AL_BAI_OPEN;
	return m[lo].file_off << 16 | (s - m[lo].s_off);
}
// The key of the record at r (its block_size field; the walk has seen that 4 + block_size bytes are there and block_size >= 32) for the descent check: al_lift_key,
// or 0 with *code set for a record whose name and CIGAR do not fit or whose refID lies beyond the list.
AL_DHD uint64_t al_bai_key(const uint8_t *r, uint32_t n_ref, uint32_t *code)
{
	const uint8_t *b = r + 4;
	const uint32_t bs = al_lift_u32(r), l_rn = b[8], n_cig = al_lift_u16(b + 12);
	const int32_t ref = (int32_t)al_lift_u32(b);
	*code = (l_rn < 1 || 32 + l_rn + 4 * n_cig > bs) ? AL_LIFT_BAD_FIT : (ref >= 0 && (uint32_t)ref >= n_ref) ? AL_LIFT_BAD_REF : 0u;
	return *code ? 0 : al_lift_key(r);
}
// One record at t + off of a text whose first byte lies at stream offset base.  0 with *o and *key set, or the code of a refusal: *o is then inert (ref -1, no
// window) and *key is the record's key where it has one.
AL_DHD uint32_t al_bai_record(const uint8_t *t, uint32_t off, uint64_t base, uint32_t n_ref, const uint32_t *ref_len, const AlBaiMember *mem, uint32_t n_mem, AlBaiRec *o, uint64_t *key)
{
	const uint8_t *r = t + off, *b = r + 4;
	const uint32_t bs = al_lift_u32(r), l_rn = b[8], n_cig = al_lift_u16(b + 12), flag = al_lift_u16(b + 14);
	uint32_t code;
	o->ref = -1; o->bin = 0; o->win = 0; o->pad = 0; o->vbeg = o->vend = 0;
	*key = al_bai_key(r, n_ref, &code);
	if (code) return code;
	const int32_t ref = (int32_t)al_lift_u32(b), pos = (int32_t)al_lift_u32(b + 4);
	o->vbeg = al_bai_voff(mem, n_mem, base + off); o->vend = al_bai_voff(mem, n_mem, base + off + 4 + (uint64_t)bs);
	if (ref < 0) return 0;
	const bool mapped = !(flag & 4);
	const int64_t beg = pos > 0 ? pos : 0, end = beg + (mapped ? al_lift_reflen(b + 32 + l_rn, n_cig) : 1);
	if (end > AL_BAI_MAX_END) return AL_BAI_BAD_BIG;
	if (mapped && end > (int64_t)ref_len[ref]) return AL_BAI_BAD_LN;
	o->ref = ref; o->bin = al_lift_reg2bin(beg, end);
	o->win = (uint32_t)(beg >> 14) | (uint32_t)((end - 1) >> 14) << 16 | (mapped ? 1u << 31 : 0u);
	return 0;
}
AL_DHD bool al_bai_head(const AlBaiRec *rec, uint32_t i) { return i == 0 || rec[i].ref != rec[i - 1].ref || rec[i].bin != rec[i - 1].bin; }

// ---- the host twin of the per-piece kernels ----------------------------------------------------------------------------------------------------------------------
// The per-contig tables both backends keep from the first piece to the last: lin[lin_off[c] + w] the smallest start offset of a record with flag 4 clear that
// touches window w of contig c (~0: none), cnt[2 c] / cnt[2 c + 1] its records with flag 4 clear / set, cnt[2 n_ref] the records with refID < 0.
struct AlBaiTables {
	std::vector<uint32_t> ref_len; std::vector<uint64_t> lin_off, lin, cnt;
	void set(const uint32_t *len, uint32_t n_ref)
	{
		ref_len.assign(len, len + n_ref); lin_off.assign((size_t)n_ref + 1, 0);
		for (uint32_t c = 0; c < n_ref; ++c) lin_off[c + 1] = lin_off[c] + al_bai_n_win(len[c]);
		lin.assign((size_t)lin_off[n_ref], ~0ull); cnt.assign(2 * (size_t)n_ref + 1, 0);
		if (ref_len.empty()) ref_len.reserve(1);
	}
};
struct AlBaiStatus { uint64_t first_bad = ~0ull; uint32_t bad_code = 0; uint64_t descents = 0, desc_off = ~0ull, last_key = 0; };
// What the kernels compute over the n records at rec_off of the text t: the refusals (the first refused record and its code; the records whose key is below the
// key before them, record 0 against prev_key when has_prev, and the smallest offset of one), the rows of the runs, and the records' share of the tables.
static inline void al_bai_piece_host(const uint8_t *t, const uint32_t *rec_off, size_t n, uint64_t base, const AlBaiMember *mem, uint32_t n_mem, bool has_prev, uint64_t prev_key,
                                     AlBaiTables &T, AlBaiStatus *st, std::vector<AlBaiRow> &rows)
{
	*st = AlBaiStatus(); rows.clear();
	const uint32_t n_ref = (uint32_t)T.ref_len.size();
	std::vector<AlBaiRec> rec(n + 1); uint64_t before = prev_key;
	for (size_t k = 0; k < n; ++k) {
		uint64_t key;
		const uint32_t code = al_bai_record(t, rec_off[k], base, n_ref, T.ref_len.data(), mem, n_mem, &rec[k], &key);
		if (code && st->first_bad == ~0ull) { st->first_bad = k; st->bad_code = code; }
		if ((k || has_prev) && key < before) { ++st->descents; if (rec_off[k] < st->desc_off) st->desc_off = rec_off[k]; }
		before = key; st->last_key = key;
	}
	if (st->first_bad != ~0ull || st->descents) return;            // (the driver refuses the piece: its rows and its share of the tables are not used)
	for (size_t k = 0; k < n; ++k) {
		const AlBaiRec &x = rec[k];
		if (al_bai_head(rec.data(), (uint32_t)k)) rows.push_back(AlBaiRow{x.ref, x.bin, x.vbeg, x.vend}); else rows.back().end = x.vend;
		if (x.ref < 0) { ++T.cnt[2 * (size_t)n_ref]; continue; }
		++T.cnt[2 * (size_t)x.ref + (x.win >> 31 ? 0 : 1)];
		if (!(x.win >> 31)) continue;
		for (uint32_t w = x.win & 0x7fff, w1 = (x.win >> 16) & 0x7fff; w <= w1; ++w) { uint64_t &v = T.lin[(size_t)T.lin_off[x.ref] + w]; if (x.vbeg < v) v = x.vbeg; }
	}
}

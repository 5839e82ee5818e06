// al_runtime.h -- per-context device state of the re-alignment pipeline (product code)
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <vector>
#include <string>
#include <thread>
#include <chrono>
#include "al_internal.h"
#include "al_stream_plan.h"
#include "al_env.h"
#include "al_devmem.h"       // al_dev_malloc / al_dev_free, al_nomem_flag, the allocation accounting

template <typename T> struct DevBuf {       // grow-only device array
	T *p = nullptr; size_t cap = 0;
	int ensure(size_t n, bool keep = false, hipStream_t s = 0, int line = __builtin_LINE(), const char *file = __builtin_FILE())
	{
		if (n <= cap) return 0;
		al_alloc_site() = AlAllocSite{file, line};
		const size_t big_div = (size_t)al_env().grow_div;
		const size_t ncap = n + (n * sizeof(T) >= ((size_t)256 << 20) ? n / big_div : n / 4) + 64;   // headroom against regrowing: an eighth for the large arrays (batches of one run differ by a few per cent), a quarter for the small
		T *np = nullptr;
		if (!keep && p) { al_dev_free(p); p = nullptr; cap = 0; }         // contents not needed: release first, so the peak is one copy
		if (al_dev_malloc((void **)&np, ncap * sizeof(T)) != hipSuccess) {
			(void)hipGetLastError();                                       // not sticky: the next launch check must not see it
			fprintf(stderr, "[airlift] device allocation of %zu bytes failed\n", ncap * sizeof(T)); al_nomem_flag() = true; return -1;
		}
		if (keep && p && cap) { if (hipMemcpyAsync(np, p, cap * sizeof(T), hipMemcpyDeviceToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return -1; }
		if (p) al_dev_free(p);
		p = np; cap = ncap;
		return 0;
	}
	void release() { if (p) al_dev_free(p); p = nullptr; cap = 0; }
};

struct AlRegOut {            // per-read result header copied back to the host
	uint32_t n_regs, reg_off;   // reg_off: index into the AlReg output array
};

// The scratch of one chaining round (al_runtime.hip: chain_tiles, chain_fallback, chain_by_segments, chain_legacy): every array those four write that is not
// a fragment's result, the temporaries of the helpers they call, and the round's device counters.  The first round (everything but the equal-x fragments, on
// main) uses the context's members of the same names; the second round (the equal-x fragments, beside the tile kernel on the side stream) has this set, so that
// neither an array's contents nor a DevBuf::ensure of one round -- it frees the old range -- touches what the other round's kernels are using.
struct AlChainScratch {
	DevBuf<uint64_t> ws_u64, u_tmp, okey_tmp, seg_first, seg_first0, vs_off, vs_res, d_uslot, v_u, v_a_off, v_first64;
	DevBuf<int32_t> ws_i32;
	DevBuf<AlAnchor> chain_tmp, v_anchors, v_chained;
	DevBuf<uint32_t> seg_cnt, seg_cnt0, seg_t1, seg_key, seg_idx, seg_ord, vs_na, vs_meta, vs_cls, d_rel, d_fragid, cmp_list, ctie, fb_list, fb2_list, fb3_list, fbk_list;
	DevBuf<uint32_t> v_na, v_nseg, v_first, v_rd_len, v_order, v_nu, lb_buf;
	DevBuf<uint8_t> scan_tmp;
	DevBuf<uint32_t> cnt;                  // [0..1] hand-backs of k_seg_merge / k_chain_order, [4..7] the tile kernel's counts, [8] flagged fragments, [10..11] their anchors (64 bits)
	void release()
	{
		ws_u64.release(); u_tmp.release(); okey_tmp.release(); seg_first.release(); seg_first0.release(); vs_off.release(); vs_res.release(); d_uslot.release(); v_u.release(); v_a_off.release(); v_first64.release();
		ws_i32.release(); chain_tmp.release(); v_anchors.release(); v_chained.release();
		seg_cnt.release(); seg_cnt0.release(); seg_t1.release(); seg_key.release(); seg_idx.release(); seg_ord.release(); vs_na.release(); vs_meta.release(); vs_cls.release(); d_rel.release(); d_fragid.release();
		cmp_list.release(); ctie.release(); fb_list.release(); fb2_list.release(); fb3_list.release(); fbk_list.release();
		v_na.release(); v_nseg.release(); v_first.release(); v_rd_len.release(); v_order.release(); v_nu.release(); lb_buf.release(); scan_tmp.release(); cnt.release();
	}
};

// The batch arrays the segment-wise chaining kernels read and write: the context's own, or those of chain_fallback's virtual batch (al_runtime.hip)
struct AlBatchPtrs { AlAnchor *anchors, *chained; uint64_t *a_off, *u; uint32_t *frag_na, *frag_first, *rd_len, *frag_nu; };

#define AL_CHAIN_WHO_N 16                  // counters of al_ctx_s::chain_who (al_runtime.hip: CW_*)
#define AL_SEED_WHO_N 32                   // counters of al_ctx_s::seed_who (al_runtime.hip: SW_*)
struct al_ctx_s {
	const al_idx_t *mi = nullptr;
	al_mapopt_t opt;
	AlParams P;
	int device = 0;
	int n_threads = 1;                    // host worker threads for packing (al_ctx_set_threads)
	// The pipeline names ten stream ROLES (AlRole, al_stream_plan.h); the context creates n_phys <= 10 streams -- as many as the process has hardware
	// queues -- and al_stream_plan() says which of them a role runs on.  Roles that share a stream run in submission order; a fork / join between two of
	// them is then plain stream order.  With ten streams (ten or more queues) every role has its own.
	//   main: the pipeline itself (`stream` below is that stream, physical 0)
	//   side: exact (serial) handling of the few fragments with equal-x anchors, next to the main pipeline; k_align in the extension stage
	//   aux0-2: more streams for stages made of independent latency-bound launches over disjoint fragments (heap merge classes, k_regs_heavy tiles)
	//   ovl0-2: stages of the seed pass that run beside the main stream's: the device-wide anchor sort next to the block sorts, the lane chaining kernels next to the tile kernel
	//   spec, spec2: the equal-x merge of giant fragments started ahead of the re-chain pass
	hipStream_t phys[AL_ROLE_N] = {};     // the streams that exist: phys[0 .. n_phys)
	uint8_t role_map[AL_ROLE_N] = {};     // role -> index into phys[]
	int n_phys = 0;
	hipStream_t stream = nullptr;         // == phys[0], the main role
	hipStream_t on(int role) const { return phys[role_map[role]]; }   // the stream a role runs on
	hipEvent_t ev_fj[2] = {};             // fork / join of the side stream inside a stage (the second chaining round, chain_post classes, DP job classes)
	hipEvent_t ev_aux[3] = {};            // join events of aux0-2
	hipEvent_t ev_ovl[5] = {};            // fork and join events of ovl0-2
	bool ovl_pending = false;             // chaining kernels in flight on ovl1: chain_tiles joins them before it reuses their scratch
	hipEvent_t ev_side[4] = {};           // [0],[1]: start / end of the side stream's work in the first pass, [2],[3]: in the re-chain pass
	// the equal-x merge of giant fragments started ahead of the re-chain pass (al_kernels_seed.hip: k_spec_build): its stream, events, slots
	hipEvent_t ev_spec[3] = {}; uint32_t n_spec = 0, spec_idle = 0, spec_batch = 0; bool spec_pending = false, spec_busy = false;   // spec_idle: batches in a row whose re-chain pass took none of the merges made ahead
	DevBuf<AlMatch> spec_match; DevBuf<uint32_t> spec_meta, spec_cnt, spec_use, spec_v32, spec_na2; DevBuf<uint64_t> spec_v64; DevBuf<AlAnchor> spec_anchors;
	float ms_side = 0;
	AlDevIndex di;
	hipEvent_t ev[ST_N + 1] = {};
	float ms_stage[ST_N] = {};
	float ms_total = 0;

	// resident batch (host mirrors kept for fetch / taps)
	int n_frag = 0, n_reads = 0;
	uint64_t n_bases = 0, mini_total = 0, seq_words = 0;
	std::vector<uint32_t> h_rd_len, h_frag_first, h_frag_hash;
	std::vector<uint64_t> h_rd_off, h_mini_off;
	std::vector<uint32_t> h_rd_seq;
	std::vector<uint8_t> h_flip;          // read was reverse-complemented for mapping (worker_for, map.c:468)

	DevBuf<uint32_t> rd_seq, rd_len, frag_first, frag_hash, mini_cnt, frag_nm, frag_na, frag_nu, rechain_list, rechain_sorted, tmp_u32;
	DevBuf<uint64_t> rd_off, mini_off, a_off, u, ws_u64, tmp_u64, tmp_u64b;
	DevBuf<uint32_t> uo;                   // per chain list entry: offset of the chain's first anchor in the fragment's range of chained[]
	DevBuf<uint64_t> big_k0, big_k1;       // key double buffer of the device-wide anchor sort (fragments above the register tiles)
	// compact copy of the fragments the tile chaining kernel hands back (al_runtime.hip: chain_fallback): a small virtual batch for the segment-wise kernels
	DevBuf<AlAnchor> v_anchors, v_chained; DevBuf<uint64_t> v_u, v_a_off, v_first64; DevBuf<uint32_t> v_na, v_nseg, v_first, v_rd_len, v_order, v_nu, fbk_list;
	DevBuf<uint64_t> d_uslot; DevBuf<uint32_t> d_rel, d_fragid, cmp_list, ctie, frag_meta, chain_cls;   // deferred segments of the tile kernel (ChainSeg direct mode), fragments whose chain lists have gaps, per-fragment tie flags
	DevBuf<int32_t> frag_rep, ws_i32;
	DevBuf<AlAnchor> mini, heap_ws, anchors, chained;
	DevBuf<AlMatch> match;
	DevBuf<unsigned long long> counters;   // [0] heap fallbacks, [1] sort-tie flags, [2] alser total, [3] n_rechain, [4..] stage specific
	DevBuf<uint8_t> scan_tmp;
	DevBuf<uint8_t> big_tmp;               // rocprim scratch of the device-wide anchor sort (it runs on ovl0, beside users of scan_tmp)
	DevBuf<uint32_t> chain_key, chain_idx, chain_idx2, tie_list, lb_buf;
	// segment-wise chaining of large fragments (al_runtime.hip: chain_by_segments) and the device-wide sort of their anchors
	DevBuf<AlAnchor> chain_tmp; DevBuf<uint64_t> u_tmp, okey_tmp, seg_first, seg_first0, vs_off, big_off, big_toff;
	DevBuf<uint64_t> vs_res;                 // two words per segment: ChainSeg::res
	DevBuf<uint32_t> seg_cnt, seg_cnt0, seg_t1, vs_na, vs_meta, vs_cls, seg_key, seg_idx, seg_ord, fb_list, fb2_list, fb3_list, big_na, big_nt, big_tent, big_cuts, tie_frags, tie_sorted, heap_cnt;
	AlChainScratch tie2;                   // the second chaining round's own scratch (the equal-x fragments, beside the first round's tile kernel)
	uint64_t n_chain_fallback = 0;
	uint64_t chain_who[AL_CHAIN_WHO_N] = {};          // which chaining kernels took how much of the last pass (al_runtime.hip: CW_*), for the al_dbg_chain tap
	DevBuf<unsigned long long> seed_cnt;                 // the al_dbg_seed tap: a count per heap-merge launch of the pass (al_runtime.hip: HF_*), in the place of counters[0]
	uint64_t seed_who[AL_SEED_WHO_N] = {};            // which anchor-sort kernels took how many fragments of the last pass (al_runtime.hip: SW_*), for the al_dbg_seed tap
	bool seed_tap_pass1 = false;                      // al_dbg_seed ran the first pass on the resident batch: its second pass may follow
	int max_qlen_sum = 0;                 // longest fragment of the resident batch
	int max_rd_len = 0;                   // longest read of the resident batch
	bool attr_chain_order = false, attr_regs_heavy = false;   // > 64 KB dynamic-LDS opt-in of two kernels: per device (hipFuncSetAttribute acts on the current device), kept per context
	bool no_taps = false;                 // the drivers' contexts: nobody reads the sorted anchors after chaining (al_dbg_* taps, candidate counting), so the alignment stage's per-mate anchor arrays take their place (16 bytes per seed hit less)
	bool dev_batch = false;               // the batch was parsed and packed on the device (al_stream.hip): no host mirrors of the read arrays
	DevBuf<uint64_t> a_off_p1; DevBuf<uint32_t> frag_na_p1; DevBuf<int32_t> frag_rep_p1;   // pass-1 snapshots when a re-chain pass ran (taps)
	uint64_t n_anchor_total = 0, n_anchor_pass1 = 0;
	double anchor_grow_hw = 1.3;          // (starts at what a repeat-rich genome needs: C4 1.26; a batch without re-seeded fragments leaves it unused) largest (anchors after the re-seeding pass) / (anchors of the first pass) this context has seen: the first pass reserves for it, so that the second does not reallocate
	uint32_t n_rechain = 0;

	// alignment stage (al_kernels_align.hip)
	DevBuf<AlReg> regs0, regs;             // fragment-level chains -> per-mate regions
	DevBuf<uint32_t> reg_cnt, cigar;
	DevBuf<uint64_t> reg_off, cig_off;
	DevBuf<uint8_t> align_ws;
	DevBuf<AlAnchor> seg_a;
	DevBuf<uint64_t> seg_u;
	uint64_t n_regs_cap_total = 0, n_cigar_cap_total = 0;
	bool ran = false;
	uint64_t stat_bytes_in = 0;
	uint32_t stat_n_slow = 0;
	unsigned long long stat_dp_jobs[10] = {}, stat_dp_tbases[10] = {};   // extension DP: jobs and target (reference window) bases per job class of the last run
	al_batch_stat_t stat;
};

int al_upload_index(const al_idx_t *mi, int device, AlDevIndex *out);
// token batches (al_runtime.hip): the counts and buffers of a batch of n_tok windows of read_len bases; the windows cut from S4 at the starts in tmp_u64b
int al_windows_prepare(al_ctx_t *c, int n_tok, int read_len);
int al_windows_cut(al_ctx_t *c, const uint32_t *S4, int n_tok, int read_len);
// tokens --gaps-bed (al_tokens.hip): the region table on the device, and tokens [t0, t0 + n_tok) of it as the resident batch -- set up by k_tok_setup, cut from
// the index's own S4.  host_mirrors: the two host arrays al_fetch_raw reads (the SAM sink) are filled.
struct AlTokDev;
AlTokDev *al_tokdev_open(int device, const uint64_t *first_tok, const uint64_t *src, const uint32_t *h_prefix, uint32_t n_rows);
void al_tokdev_close(AlTokDev *T);
int al_batch_upload_tokens(al_ctx_t *c, const AlTokDev *T, uint64_t t0, int n_tok, int read_len, int skip, bool host_mirrors);
float al_tokdev_ms(const AlTokDev *T);     // k_tok_setup's device time so far (HIP events)
int al_tokdev_fetch_s4(al_ctx_t *c, std::vector<uint32_t> &S4);   // the index's packed reference, device -> host (a device-built index has no host copy)
void al_ctx_no_taps(al_ctx_t *c);         // see al_ctx_s::no_taps
int al_run_align_stage(al_ctx_t *c);      // al_kernels_align.hip: KA (regs) + K5 (extension, MAPQ, pairing)
// MD:Z / cs:Z tags of a batch's compacted records (--MD / --cs, al_kernels_tags.hip): value bytes of output record k at arena[off[k] .. off[k + 1])
struct AlTagBufs { DevBuf<uint32_t> len; DevBuf<uint64_t> off; DevBuf<char> arena; uint64_t bytes = 0; };
int al_run_tag_stage(al_ctx_t *c, const AlReg *out, const uint64_t *out_off, uint64_t n_out, const uint32_t *arena, AlTagBufs &T);
// --eqx (al_kernels_tags.hip): the records' M operations rewritten as =/X runs into a fresh arena E (E.bytes = its words), records updated in place
int al_run_eqx_stage(al_ctx_t *c, AlReg *out, const uint64_t *out_off, uint64_t n_out, const uint32_t *arena, AlTagBufs &E);
int al_run_tags(al_ctx_t *c);             // al_kernels_align.hip: the =/X pass and the tag stage on the last run's records, when the options ask for them
// a map-only run (no base-level alignment): PAF output without AL_F_CIGAR; only under AL_F_OUT_PAF is AL_F_CIGAR looked at (airlift.h)
static inline bool al_map_only(int64_t flag) { return (flag & AL_F_OUT_PAF) && !(flag & AL_F_CIGAR); }
static inline int al_tag_kind(int64_t flag) { return al_map_only(flag) ? 0 : (flag & AL_F_OUT_MD) ? 1 : (flag & AL_F_OUT_CS) ? 2 : 0; }   // 0 none, 1 MD, 2 cs (MD wins, format.c:533)
int al_fetch_align(al_ctx_t *c, int *n_regs, al_reg1_t **regs, int *rep_len);
void al_align_grow_arena(al_ctx_t *c);
int al_align_run_to_fit(al_ctx_t *c, int *reruns);   // al_kernels_align.hip: al_run_align_stage, run again with twice the CIGAR arena while it overflows

template <typename T> struct PinnedVec {    // grow-only page-locked host array (fast, asynchronous-capable D2H target)
	T *p = nullptr; size_t n = 0, cap = 0;
	PinnedVec() {}
	PinnedVec(const PinnedVec &) = delete; PinnedVec &operator=(const PinnedVec &) = delete;
	~PinnedVec() { if (p) (void)hipHostFree(p); }
	int resize(size_t m)
	{
		if (m > cap) {
			const size_t ncap = m + m / 4 + 1024;
			T *np = nullptr;
			const auto t0__ = std::chrono::steady_clock::now();
			const hipError_t e__ = hipHostMalloc((void **)&np, ncap * sizeof(T), hipHostMallocDefault);
			{ AlAllocStat &a = al_alloc_stat(); a.host_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0__).count(); a.host_bytes += (long long)(ncap * sizeof(T)); ++a.host_calls; }
			if (e__ != hipSuccess) { fprintf(stderr, "[airlift] hipHostMalloc of %zu bytes failed\n", ncap * sizeof(T)); return -1; }
			if (p) (void)hipHostFree(p);
			p = np; cap = ncap;
		}
		n = m; return 0;
	}
	T *data() { return p; } const T *data() const { return p; }
	size_t size() const { return n; }
	T &operator[](size_t i) { return p[i]; } const T &operator[](size_t i) const { return p[i]; }
};

struct AlRawResult {         // flat host copy of one batch's results (no per-record allocation); reusable across batches
	PinnedVec<uint64_t> off;              // per read: first record in out[]; off[n_reads] = total
	PinnedVec<AlReg> out;
	PinnedVec<uint32_t> arena;            // CIGAR words of records with more than 4 operations
	PinnedVec<int32_t> rep;               // per fragment repeat length
	std::vector<uint8_t> flip;            // read was mapped reverse-complemented
	std::vector<uint32_t> rd_len;
	int tag_kind = 0;                     // al_tag_kind() of the run's options: tag values of record k at tag[tag_off[k] .. tag_off[k + 1])
	PinnedVec<uint64_t> tag_off;
	PinnedVec<char> tag;
};
int  al_fetch_raw(al_ctx_t *c, AlRawResult &R);
// al_write_sam with the file drivers' output options (al_api.cpp): AL_F_SOFTCLIP, and the record's MD:Z / cs:Z value (tag, tag_len) by al_tag_kind(opt_flag)
int  al_write_sam_ex(char *buf, size_t cap, const al_idx_t *mi, const char *qname, int l_seq, const char *seq, const char *qual,
                     int seg_idx, int reg_idx, int n_seg, const int *n_regss, const al_reg1_t *const *regss, const char *rg_id, int rep_len,
                     int64_t opt_flag, const char *tag, int tag_len);
// al_write_paf with the tag value given by length (the device's tag arena is not NUL-terminated)
int  al_write_paf_ex(char *buf, size_t cap, const al_idx_t *mi, const char *qname, int l_seq, const al_reg1_t *r, int64_t opt_flag, int rep_len, const char *tag, int tag_len);
void al_reg_from_raw(const AlRawResult &R, int read, int k, al_reg1_t &q);

// host worker pool helper: fn(lo, hi, thread) over [0, n) split into contiguous ranges
template <class F> static inline void al_parallel_for(int n_threads, size_t n, F fn)
{
	if (n_threads <= 1 || n < 2) { fn((size_t)0, n, 0); return; }
	const size_t nt = (size_t)n_threads < n ? (size_t)n_threads : n;
	std::vector<std::thread> th; th.reserve(nt);
	for (size_t t = 0; t < nt; ++t) th.emplace_back(fn, n * t / nt, n * (t + 1) / nt, (int)t);
	for (auto &x : th) x.join();
}

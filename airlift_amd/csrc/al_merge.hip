// al_merge.hip -- `merge`: 2 to 8 coordinate-sorted BAMs merged into one on the GPU (the function: al_dev_merge.h; the driver: al_merge.h).
//
// Per refill of an input's window, on the input's own stream:
//   k_bam_walk        al_dev_walk.h, as `lift` launches it: the record offsets of the window's text
//   k_merge_key       lane per record: the fixed fields read byte-wise (records are not aligned), refID and next_refID range-checked against the input's n_ref,
//                     translated through the input's table and patched in place; the key and the record's length written; the first refused record by atomicMin
//   k_merge_descents  lane per record: key[i] < key[i - 1] counted per wavefront with one atomic per wavefront, index 0 judged against the last key of the same
//                     input's window before; the smallest offset of such a record by atomicMin.  (A kernel of its own, as k_lift_descents is: a lane of
//                     k_merge_key cannot read its predecessor's refID while that record's own lane may be patching it.)
// Per round, on the merge stream:
//   k_merge_bounds    lane per input: al_merge_emit_count, a binary search over the window's keys from the cursor; the k counts and their total come down with
//                     one small copy
//   k_merge_runs      lane per emitted record: (key, tag) of the k runs laid out one behind the other, tag = input << 28 | record index in the window
//   k_merge_part      lane per output tile of AL_MERGE_TILE elements: the merge path's split of the tile's diagonal; on equal keys it takes from the first run
//   k_merge_tile      block per output tile: both shares of (key, tag) into LDS, every lane finds the split of its own diagonal there and merges AL_MERGE_VT
//                     consecutive outputs into registers; the outputs go back through LDS so that the stores to global memory are coalesced
//                     k runs take ceil(log2 k) passes over pairs of ADJACENT runs, the lower inputs on the left, an odd run out copied through: "the first run
//                     wins ties" in every pass is then "the earlier input wins ties" in the result
//   k_merge_plen      lane per merged index: the record's length; al_stream_scan_excl_u64 over them makes the offsets
//   k_merge_gather    16 lanes per record: the tag's input field chooses the text and the offset table (a by-value struct of 8 pointers each)
// Output: with --gpu-deflate AlBgzf::write_device from the packed buffer (fetch + write when it declines), otherwise a copy down into page-locked memory, on a
// stream of its own, and AlBgzf::write; there are two packed buffers, so a round's copy down and host deflate run beside the next round's kernels.
//
// AL_MERGE_TILE = 1024 = 256 lanes x AL_MERGE_VT 4.  A block holds 1024 x (8 + 4) = 12 KiB of LDS, so the 160 KiB of a CU would take 13 blocks and LDS is not the
// limit; 256 lanes are 4 wavefronts, one per SIMD, and the 32-wavefront cap of a CU allows 8 blocks, which is what the kernel is meant to reach: a lane holds 4
// keys and 4 tags beside its cursors, far below the 64 VGPRs that 8 wavefronts per SIMD allow.  A larger AL_MERGE_VT shortens the binary searches per output but
// lengthens the serial merge whose LDS reads depend on each other; 4 is the guess that keeps many wavefronts in flight to hide those reads.  These values are
// UNMEASURED: no profile of this kernel exists yet.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <atomic>
#include <memory>
#include <string>
#include "al_internal.h"
#include "al_device.h"
#include "al_runtime.h"
#include "al_stream.h"
#include "al_dev_inflate.h"
#include "al_bam.h"
#include "al_merge.h"
#include "al_bai.h"
#include "al_dev_walk.h"
#include "al_env.h"
#include "../../include/airlift.h"

__global__ void __launch_bounds__(256)
k_merge_key(uint8_t *__restrict__ t, const uint32_t *__restrict__ rec_off, uint32_t n_rec, const int32_t *__restrict__ map, uint32_t n_ref, uint64_t *__restrict__ key, uint32_t *__restrict__ rlen,
            unsigned long long *__restrict__ first_bad)
{
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n_rec) return;
	uint64_t k; uint32_t len;
	if (al_merge_record(t + rec_off[r], map, n_ref, &k, &len)) atomicMin(first_bad, (unsigned long long)r);
	key[r] = k; rlen[r] = len;
}
// cnt[0]: descents, cnt[1]: the smallest offset of a record below its predecessor
__global__ void __launch_bounds__(256)
k_merge_descents(const uint64_t *__restrict__ key, const uint32_t *__restrict__ rec_off, uint32_t n_rec, uint32_t has_prev, uint64_t prev_key, unsigned long long *__restrict__ cnt)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	const bool d = i < n_rec && (i ? key[i] < key[i - 1] : (has_prev && key[0] < prev_key));
	const unsigned long long m = __ballot(d);
	if ((threadIdx.x & 63) == 0 && m) atomicAdd(cnt, (unsigned long long)__popcll(m));
	if (d) atomicMin(cnt + 1, (unsigned long long)rec_off[i]);
}
// out[0, k): the records each input emits, out[AL_MERGE_MAX_IN]: their total
__global__ void __launch_bounds__(64)
k_merge_bounds(AlMergeWins W, uint32_t *__restrict__ out)
{
	__shared__ uint32_t c[AL_MERGE_MAX_IN];
	const uint32_t i = threadIdx.x;
	if (i < AL_MERGE_MAX_IN) c[i] = i < W.k ? al_merge_emit_count(W, i) : 0u;
	__syncthreads();
	if (i < AL_MERGE_MAX_IN) out[i] = c[i];
	if (i == 0) { uint32_t s = 0; for (uint32_t j = 0; j < AL_MERGE_MAX_IN; ++j) s += c[j]; out[AL_MERGE_MAX_IN] = s; }
}
struct AlMergeRuns { uint32_t off[AL_MERGE_MAX_IN + 1]; };              // run i is elements [off[i], off[i + 1]) of the round
__global__ void __launch_bounds__(256)
k_merge_runs(AlMergeWins W, AlMergeRuns R, uint64_t *__restrict__ key, uint32_t *__restrict__ tag)
{
	const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= R.off[W.k]) return;
	uint32_t i = 0;
	while (i + 1 < W.k && e >= R.off[i + 1]) ++i;
	const uint32_t x = W.w[i].cur + (e - R.off[i]);                   // (< W.w[i].n: the counts come from al_merge_emit_count)
	key[e] = W.w[i].key[x]; tag[e] = i << AL_MERGE_TAG_BITS | x;
}
// split[t], t in [0, n_tiles]: how many of the first min(t * AL_MERGE_TILE, na + nb) outputs come from a
__global__ void __launch_bounds__(256)
k_merge_part(const uint64_t *__restrict__ a, uint32_t na, const uint64_t *__restrict__ b, uint32_t nb, uint32_t n_tiles, uint32_t *__restrict__ split)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t > n_tiles) return;
	const uint64_t d = (uint64_t)t * AL_MERGE_TILE;
	split[t] = al_merge_path(a, na, b, nb, d < (uint64_t)na + nb ? (uint32_t)d : na + nb);
}
__global__ void __launch_bounds__(AL_MERGE_THREADS)
k_merge_tile(const uint64_t *__restrict__ ka, const uint32_t *__restrict__ ta, uint32_t na, const uint64_t *__restrict__ kb, const uint32_t *__restrict__ tb, uint32_t nb,
             const uint32_t *__restrict__ split, uint64_t *__restrict__ ko, uint32_t *__restrict__ to)
{
	__shared__ uint64_t sk[AL_MERGE_TILE];
	__shared__ uint32_t st[AL_MERGE_TILE];
	const uint32_t n = na + nb, d0 = blockIdx.x * AL_MERGE_TILE, d1 = d0 + AL_MERGE_TILE < n ? d0 + AL_MERGE_TILE : n;
	const uint32_t a0 = split[blockIdx.x], a1 = split[blockIdx.x + 1], b0 = d0 - a0, la = a1 - a0, m = d1 - d0, lb = m - la;
	for (uint32_t j = threadIdx.x; j < m; j += AL_MERGE_THREADS) {
		if (j < la) { sk[j] = ka[a0 + j]; st[j] = ta[a0 + j]; }
		else { sk[j] = kb[b0 + (j - la)]; st[j] = tb[b0 + (j - la)]; }
	}
	__syncthreads();
	const uint32_t d = threadIdx.x * AL_MERGE_VT < m ? threadIdx.x * AL_MERGE_VT : m;
	uint32_t x = al_merge_path(sk, la, sk + la, lb, d), y = d - x;
	uint64_t rk[AL_MERGE_VT]; uint32_t rt[AL_MERGE_VT];
	_Pragma("unroll")
	for (uint32_t v = 0; v < AL_MERGE_VT; ++v) {
		rk[v] = 0; rt[v] = 0;
		if (d + v < m) {
			const bool from_a = y >= lb || (x < la && sk[x] <= sk[la + y]);
			const uint32_t s = from_a ? x : la + y;
			rk[v] = sk[s]; rt[v] = st[s];
			if (from_a) ++x; else ++y;
		}
	}
	__syncthreads();
	_Pragma("unroll")
	for (uint32_t v = 0; v < AL_MERGE_VT; ++v) if (d + v < m) { sk[d + v] = rk[v]; st[d + v] = rt[v]; }
	__syncthreads();
	for (uint32_t j = threadIdx.x; j < m; j += AL_MERGE_THREADS) { ko[d0 + j] = sk[j]; to[d0 + j] = st[j]; }
}
__global__ void __launch_bounds__(256)
k_merge_plen(const uint32_t *__restrict__ tag, uint32_t n, AlMergePtrs P, uint32_t *__restrict__ plen)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) { const uint32_t t = tag[i]; plen[i] = P.rlen[t >> AL_MERGE_TAG_BITS][t & AL_MERGE_TAG_MASK]; }
	else if (i == n) plen[i] = 0;                                       // (the scan's last element: the total)
}
__global__ void __launch_bounds__(256)
k_merge_gather(const uint32_t *__restrict__ tag, uint32_t n, AlMergePtrs P, const uint32_t *__restrict__ plen, const uint64_t *__restrict__ off, uint8_t *__restrict__ packed)
{
	const uint32_t i = blockIdx.x * 16 + (threadIdx.x >> 4), l = threadIdx.x & 15;
	if (i >= n) return;
	const uint32_t t = tag[i], in = t >> AL_MERGE_TAG_BITS;
	const uint8_t *src = P.txt[in] + P.rec_off[in][t & AL_MERGE_TAG_MASK];
	const uint32_t len = plen[i];
	uint8_t *o = packed + off[i];
	for (uint32_t j = l; j < len; j += 16) o[j] = src[j];
}

namespace {

#define MERGE_CHECK(x) AL_HIP_CHECK_AS("merge", x)
static inline double merge_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct AlMergeDevBackend : AlMergeBackend {
	int device = 0, k = 0; bool open_ok = false;
	std::atomic<size_t> own_acct{0}, *acct = &own_acct, *acct_before = nullptr;      // the account every device range of the backend is booked on
	AlStreamSlot S[AL_MERGE_MAX_IN]; int at[AL_MERGE_MAX_IN] = {};
	DevBuf<uint32_t> rec_off[AL_MERGE_MAX_IN], rlen[AL_MERGE_MAX_IN]; DevBuf<uint64_t> key[AL_MERGE_MAX_IN]; DevBuf<int32_t> d_map[AL_MERGE_MAX_IN]; uint32_t n_ref[AL_MERGE_MAX_IN] = {};
	DevBuf<unsigned long long> cnt[AL_MERGE_MAX_IN];                     // first_bad, descents, desc_off; the walk's three words behind them
	DevBuf<uint32_t> d_bounds, mt[2], ft[2], split, plen; DevBuf<uint64_t> mk[2], fk[2], poff; DevBuf<uint8_t> packed[2];
	PinnedVec<uint8_t> h_packed[2];
	unsigned long long *h_cnt = nullptr;                                // page-locked: 8 words per input, then 16 for the rounds
	hipStream_t M = nullptr, Cp = nullptr; hipEvent_t ev_g[2] = {nullptr, nullptr}, ev_c[2] = {nullptr, nullptr};   // per packed buffer: its gather is done, its copy down is done
	int gather_pending = -1;                                            // the packed buffer whose gather has not been waited for
	size_t n_merged[2] = {0, 0};
	double up_s = 0, walk_s = 0, key_s = 0, merge_s = 0, gather_s = 0, down_s = 0;

	const char *name() const override { return "k_merge"; }
	// 0, or 1 when there is no usable device or it refuses the memory (nothing is left allocated after the destructor)
	int open(int dev, int n_in, size_t cap_in, size_t cap_mem)
	{
		int n_dev = 0;
		if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) { (void)hipGetLastError(); return 1; }
		device = dev < 0 ? 0 : dev; k = n_in;
		if (device >= n_dev || hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return 1; }
		acct_before = al_acct(); al_acct() = acct; open_ok = true;
		for (int i = 0; i < k; ++i) {
			if (al_stream_slot_init(S[i], nullptr, device, 2)) return 1;
			if (cnt[i].ensure(8)) return 1;
			if (cap_in && al_stream_bgzf_init(S[i], cap_in, cap_mem)) return 1;
		}
		if (d_bounds.ensure(AL_MERGE_MAX_IN + 8)) return 1;
		if (hipStreamCreateWithFlags(&M, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&Cp, hipStreamNonBlocking) != hipSuccess ||
		    hipEventCreateWithFlags(&ev_g[0], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ev_g[1], hipEventDisableTiming) != hipSuccess ||
		    hipEventCreateWithFlags(&ev_c[0], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ev_c[1], hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return 1; }
		if (hipHostMalloc((void **)&h_cnt, (8 * AL_MERGE_MAX_IN + 16) * 8, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); h_cnt = nullptr; return 1; }
		return 0;
	}
	~AlMergeDevBackend() override
	{
		if (!open_ok) return;
		(void)hipSetDevice(device);
		if (M) (void)hipStreamSynchronize(M);
		if (Cp) (void)hipStreamSynchronize(Cp);
		for (int i = 0; i < AL_MERGE_MAX_IN; ++i) {
			if (S[i].io) (void)hipStreamSynchronize(S[i].io);
			rec_off[i].release(); rlen[i].release(); key[i].release(); d_map[i].release(); cnt[i].release();
			al_stream_slot_destroy(S[i]);
		}
		for (int s = 0; s < 2; ++s) { mt[s].release(); ft[s].release(); mk[s].release(); fk[s].release(); packed[s].release(); }
		d_bounds.release(); split.release(); plen.release(); poff.release();
		if (M) (void)hipStreamDestroy(M); if (Cp) (void)hipStreamDestroy(Cp);
		for (int s = 0; s < 2; ++s) { if (ev_g[s]) (void)hipEventDestroy(ev_g[s]); if (ev_c[s]) (void)hipEventDestroy(ev_c[s]); }
		if (h_cnt) (void)hipHostFree(h_cnt);
		al_acct() = acct_before;
	}
	size_t held() const override { return acct->load(); }

	int set_map(int i, const int32_t *m, uint32_t nr) override
	{
		MERGE_CHECK(hipSetDevice(device));
		if (d_map[i].ensure((size_t)nr + 1)) return -1;
		if (nr) MERGE_CHECK(hipMemcpy(d_map[i].p, m, (size_t)nr * 4, hipMemcpyHostToDevice));
		n_ref[i] = nr;
		return 0;
	}
	// The round before may still be gathering from this input's arrays: they are released and written from here on, so the gather is waited for.
	int begin(int i, size_t cap) override
	{
		MERGE_CHECK(hipSetDevice(device));
		if (gather_pending >= 0) { MERGE_CHECK(hipEventSynchronize(ev_g[gather_pending])); gather_pending = -1; }
		at[i] ^= 1;
		return al_stream_begin_text(S[i], at[i], cap + 2 * AL_LIFT_W) ? -1 : 0;     // (room for k_bam_walk to load whole windows)
	}
	int room(int i, uint64_t n) const { if (S[i].txt_n[at[i]] + n + 16 > S[i].txt[at[i]].cap) { fprintf(stderr, "[airlift] merge: text buffer too small\n"); return -1; } return 0; }
	int carry(int i, uint64_t off, uint64_t n) override
	{
		if (n == 0) return 0;
		const int a = at[i], o = a ^ 1;
		if (room(i, n) || off + n > S[i].txt_n[o]) return -1;
		MERGE_CHECK(hipMemcpyAsync(S[i].txt[a].p + S[i].txt_n[a], S[i].txt[o].p + off, n, hipMemcpyDeviceToDevice, S[i].io));
		S[i].txt_n[a] += n;
		return 0;
	}
	int append(int i, const uint8_t *p, size_t n) override
	{
		if (n == 0) return 0;
		const int a = at[i];
		if (room(i, n)) return -1;
		MERGE_CHECK(hipMemcpyAsync(S[i].txt[a].p + S[i].txt_n[a], p, n, hipMemcpyHostToDevice, S[i].io));
		MERGE_CHECK(hipStreamSynchronize(S[i].io));
		S[i].txt_n[a] += n;
		return 0;
	}
	int append_bgzf(int i, const uint8_t *b, size_t n_in, const AlInfMember *mem, size_t n_mem, uint64_t n_out, size_t *bad, uint32_t *bad_status) override
	{
		const double t0 = merge_now(), k0 = S[i].bz.kernel_s;
		const int r = al_stream_append_bgzf(S[i], at[i], b, n_in, mem, n_mem, n_out, bad, bad_status);
		up_s += merge_now() - t0 - (S[i].bz.kernel_s - k0);
		return r;
	}
	uint64_t text_bytes(int i) const override { return S[i].txt_n[at[i]]; }
	int run(int i, uint64_t start, bool has_prev, uint64_t prev_key, AlMergePiece *r) override
	{
		AlStreamSlot &X = S[i]; hipStream_t st = X.io; const int a = at[i];
		MERGE_CHECK(hipSetDevice(device));
		*r = AlMergePiece();
		const uint64_t n = X.txt_n[a];
		if (n >= (1ull << 31) || start > n) { fprintf(stderr, "[airlift] merge: a text of %llu bytes\n", (unsigned long long)n); return -1; }
		const double t0 = merge_now();
		if (rec_off[i].ensure((size_t)(n / 36) + 64)) return -1;          // (a record takes at least 36 bytes)
		unsigned long long *h = h_cnt + 8 * i; uint32_t *hw = (uint32_t *)(h + 4);
		h[0] = ~0ull; h[1] = 0; h[2] = ~0ull; h[3] = 0;
		MERGE_CHECK(hipMemcpyAsync(cnt[i].p, h, 32, hipMemcpyHostToDevice, st));
		hipLaunchKernelGGL(k_bam_walk, dim3(1), dim3(64), 0, st, X.txt[a].p, (uint32_t)n, (uint32_t)std::min<size_t>(X.txt[a].cap, 0xfffffff0u), (uint32_t)start, rec_off[i].p, (uint32_t *)(cnt[i].p + 4));
		MERGE_CHECK(hipMemcpyAsync(hw, cnt[i].p + 4, 12, hipMemcpyDeviceToHost, st));
		MERGE_CHECK(hipStreamSynchronize(st));
		MERGE_CHECK(hipGetLastError());
		const double t1 = merge_now(); walk_s += t1 - t0;
		const uint32_t nr = hw[0];
		r->n_rec = nr; r->consumed = hw[1]; r->walk_bad = hw[2];
		if (key[i].ensure((size_t)nr + 2) || rlen[i].ensure((size_t)nr + 2)) return -1;
		if (nr) {
			hipLaunchKernelGGL(k_merge_key, dim3((nr + 255) / 256), dim3(256), 0, st, X.txt[a].p, rec_off[i].p, nr, d_map[i].p, n_ref[i], key[i].p, rlen[i].p, cnt[i].p);
			hipLaunchKernelGGL(k_merge_descents, dim3((nr + 255) / 256), dim3(256), 0, st, key[i].p, rec_off[i].p, nr, has_prev ? 1u : 0u, prev_key, cnt[i].p + 1);
			MERGE_CHECK(hipMemcpyAsync(h, cnt[i].p, 24, hipMemcpyDeviceToHost, st));
			MERGE_CHECK(hipMemcpyAsync(h + 3, key[i].p + (nr - 1), 8, hipMemcpyDeviceToHost, st));
			MERGE_CHECK(hipStreamSynchronize(st));
			MERGE_CHECK(hipGetLastError());
			r->first_bad = h[0]; r->descents = h[1]; r->desc_off = h[2]; r->last_key = h[3];
			if (r->first_bad != ~0ull) { uint32_t off = 0; MERGE_CHECK(hipMemcpy(&off, rec_off[i].p + r->first_bad, 4, hipMemcpyDeviceToHost)); r->bad_off = off; }
		}
		key_s += merge_now() - t1;
		return 0;
	}
	void wins(const uint32_t *cur, const uint32_t *n, const uint8_t *eof, int kk, AlMergeWins &W) const
	{
		memset(&W, 0, sizeof(W)); W.k = (uint32_t)kk;
		for (int i = 0; i < kk; ++i) W.w[i] = AlMergeWin{key[i].p, cur[i], n[i], eof ? (uint32_t)eof[i] : 0u};
	}
	int bounds(const uint32_t *cur, const uint32_t *n, const uint8_t *eof, int kk, uint32_t *c, uint64_t *total) override
	{
		MERGE_CHECK(hipSetDevice(device));
		const double t0 = merge_now();
		AlMergeWins W; wins(cur, n, eof, kk, W);
		uint32_t *h = (uint32_t *)(h_cnt + 8 * AL_MERGE_MAX_IN);
		hipLaunchKernelGGL(k_merge_bounds, dim3(1), dim3(64), 0, M, W, d_bounds.p);
		MERGE_CHECK(hipMemcpyAsync(h, d_bounds.p, (AL_MERGE_MAX_IN + 1) * 4, hipMemcpyDeviceToHost, M));
		MERGE_CHECK(hipStreamSynchronize(M));
		MERGE_CHECK(hipGetLastError());
		for (int i = 0; i < kk; ++i) { c[i] = h[i]; if ((uint64_t)cur[i] + c[i] > n[i]) { fprintf(stderr, "[airlift] merge: a count beyond the window\n"); return -1; } }
		*total = h[AL_MERGE_MAX_IN];
		merge_s += merge_now() - t0;
		return 0;
	}
	int merge(int s, const uint32_t *cur, const uint32_t *c, int kk, bool packed_down, AlMergeRound *r) override
	{
		MERGE_CHECK(hipSetDevice(device));
		const double t0 = merge_now();
		AlMergeWins W; wins(cur, c, nullptr, kk, W);                     // (k_merge_runs reads key and cur)
		AlMergeRuns R; uint64_t tot = 0;
		for (int i = 0; i <= AL_MERGE_MAX_IN; ++i) { R.off[i] = (uint32_t)tot; if (i < kk) tot += c[i]; }
		if (tot >= (1ull << 31)) { fprintf(stderr, "[airlift] merge: a round of 2^31 records or more; use a smaller --piece\n"); return -1; }
		const uint32_t n = (uint32_t)tot;
		std::vector<uint32_t> off;                                       // the runs that hold a record, as offsets; off.back() = n
		for (int i = 0; i < kk; ++i) if (c[i]) off.push_back(R.off[i]);
		off.push_back(n);
		size_t runs = off.size() - 1; int passes = 0;
		for (size_t q = runs; q > 1; q = (q + 1) / 2) ++passes;
		if (fk[s].ensure((size_t)n + 2) || ft[s].ensure((size_t)n + 2) || plen.ensure((size_t)n + 2) || poff.ensure((size_t)n + 2)) return -1;
		if (passes > 0 && (mk[0].ensure((size_t)n + 2) || mt[0].ensure((size_t)n + 2))) return -1;
		if (passes > 1 && (mk[1].ensure((size_t)n + 2) || mt[1].ensure((size_t)n + 2))) return -1;
		if (passes > 0 && split.ensure((size_t)n / AL_MERGE_TILE + 8)) return -1;
		uint64_t *sk = passes ? mk[0].p : fk[s].p; uint32_t *stg = passes ? mt[0].p : ft[s].p; int cur_buf = 0;
		hipLaunchKernelGGL(k_merge_runs, dim3((n + 255) / 256), dim3(256), 0, M, W, R, sk, stg);
		for (int p = 0; p < passes; ++p) {
			const bool last = p + 1 == passes;
			uint64_t *dk = last ? fk[s].p : mk[cur_buf ^ 1].p; uint32_t *dt = last ? ft[s].p : mt[cur_buf ^ 1].p;
			std::vector<uint32_t> next;
			for (size_t q = 0; q + 1 < off.size(); q += 2) {
				next.push_back(off[q]);
				const uint32_t o = off[q];
				if (q + 2 < off.size()) {
					const uint32_t na = off[q + 1] - o, nb = off[q + 2] - off[q + 1], tiles = (na + nb + AL_MERGE_TILE - 1) / AL_MERGE_TILE;
					hipLaunchKernelGGL(k_merge_part, dim3((tiles + 256) / 256), dim3(256), 0, M, sk + o, na, sk + o + na, nb, tiles, split.p);
					hipLaunchKernelGGL(k_merge_tile, dim3(tiles), dim3(AL_MERGE_THREADS), 0, M, sk + o, stg + o, na, sk + o + na, stg + o + na, nb, split.p, dk + o, dt + o);
				} else {                                                     // an odd run out passes through
					const uint32_t na = off[q + 1] - o;
					MERGE_CHECK(hipMemcpyAsync(dk + o, sk + o, (size_t)na * 8, hipMemcpyDeviceToDevice, M));
					MERGE_CHECK(hipMemcpyAsync(dt + o, stg + o, (size_t)na * 4, hipMemcpyDeviceToDevice, M));
				}
			}
			next.push_back(n); off.swap(next);
			sk = dk; stg = dt; cur_buf ^= 1;
		}
		AlMergePtrs P; memset(&P, 0, sizeof(P));
		for (int i = 0; i < kk; ++i) { P.txt[i] = S[i].txt[at[i]].p; P.rec_off[i] = rec_off[i].p; P.rlen[i] = rlen[i].p; }
		hipLaunchKernelGGL(k_merge_plen, dim3((n + 256) / 256), dim3(256), 0, M, ft[s].p, n, P, plen.p);
		if (al_stream_scan_excl_u64(S[0], plen.p, poff.p, (size_t)n + 1, M)) return -1;
		unsigned long long *h = h_cnt + 8 * AL_MERGE_MAX_IN + 8;
		MERGE_CHECK(hipMemcpyAsync(h, poff.p + n, 8, hipMemcpyDeviceToHost, M));
		MERGE_CHECK(hipStreamSynchronize(M));
		MERGE_CHECK(hipGetLastError());
		const double t1 = merge_now(); merge_s += t1 - t0;
		const uint64_t bytes = h[0];
		r->n = n; r->bytes = bytes; n_merged[s] = n;
		if (packed[s].ensure((size_t)bytes + 16) || (packed_down && h_packed[s].resize((size_t)bytes + 1))) return -1;
		if (n) hipLaunchKernelGGL(k_merge_gather, dim3((n + 15) / 16), dim3(256), 0, M, ft[s].p, n, P, plen.p, poff.p, packed[s].p);
		MERGE_CHECK(hipEventRecord(ev_g[s], M));
		gather_pending = s;
		MERGE_CHECK(hipStreamWaitEvent(Cp, ev_g[s], 0));
		if (packed_down && bytes) MERGE_CHECK(hipMemcpyAsync(h_packed[s].data(), packed[s].p, (size_t)bytes, hipMemcpyDeviceToHost, Cp));
		MERGE_CHECK(hipEventRecord(ev_c[s], Cp));
		MERGE_CHECK(hipGetLastError());
		return 0;
	}
	int finish(int s, const uint8_t **p) override
	{
		const double t0 = merge_now();
		MERGE_CHECK(hipEventSynchronize(ev_g[s]));
		if (gather_pending == s) gather_pending = -1;
		const double t1 = merge_now(); gather_s += t1 - t0;
		MERGE_CHECK(hipEventSynchronize(ev_c[s]));
		MERGE_CHECK(hipGetLastError());
		down_s += merge_now() - t1;
		*p = h_packed[s].data();
		return 0;
	}
	// the packed records of a slot after finish(), for a slot whose bytes did not come down with the merge
	int fetch_packed(int s, const AlMergeRound &r, const uint8_t **p)
	{
		if (h_packed[s].resize((size_t)r.bytes + 1)) return -1;
		const double t0 = merge_now();
		if (r.bytes) MERGE_CHECK(hipMemcpy(h_packed[s].data(), packed[s].p, (size_t)r.bytes, hipMemcpyDeviceToHost));
		down_s += merge_now() - t0;
		*p = h_packed[s].data();
		return 0;
	}
	int fetch_merged(int s, uint32_t *t, uint64_t *kk, size_t n) override
	{
		if (n > n_merged[s]) return -1;
		if (n) { MERGE_CHECK(hipMemcpy(t, ft[s].p, n * 4, hipMemcpyDeviceToHost)); MERGE_CHECK(hipMemcpy(kk, fk[s].p, n * 8, hipMemcpyDeviceToHost)); }
		return 0;
	}
	void *host_buffer(size_t n) override { void *p = nullptr; if (hipHostMalloc(&p, n, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; } return p; }
	void host_buffer_free(void *p) override { (void)hipHostFree(p); }
	void stat(AlMergeRun &st) override
	{
		st.up_s += up_s; st.walk_s += walk_s; st.key_s += key_s; st.merge_s += merge_s; st.gather_s += gather_s; st.down_s += down_s;
		for (int i = 0; i < k; ++i) st.inflate_s += S[i].bz.kernel_s;
	}
};

struct MergeFiles { std::vector<int> fd; ~MergeFiles() { for (int f : fd) if (f >= 0) close(f); } };

// One attempt with one backend.  0; -1; -2 malformed or unsorted input; *nomem: the device refused memory (the caller runs the twin)
int merge_once(const char *const *bam_in, int n_in, const MergeFiles &F, const std::vector<AlLiftHeader> &H, const AlMergeHeaders &MH, const std::vector<uint64_t> &file_off, const std::vector<uint64_t> &out_off,
               const std::vector<uint64_t> &start, const char *bam_out, bool host_backend, bool gpu_deflate, int device, int n_threads, int level, size_t piece_bytes, AlMergeRun &run, const char **backend,
               double *deflate_s, std::atomic<size_t> &acct, bool *nomem)
{
	*nomem = false;
	const size_t zpiece = (size_t)al_env().inflate_piece_kb << 10, zcap = 2 * zpiece + 65536, zmem = zcap / 64 + 1024;
	if (piece_bytes == 0) piece_bytes = std::max((size_t)8 << 20, 4 * zpiece);
	if (piece_bytes >= ((size_t)1 << 29)) piece_bytes = (size_t)1 << 29;
	std::unique_ptr<AlMergeBackend> B; AlMergeDevBackend *D = nullptr;
	if (!host_backend) {
		std::unique_ptr<AlMergeDevBackend> d(new AlMergeDevBackend()); d->acct = &acct;
		if (d->open(device, n_in, zcap, zmem) == 0) { D = d.get(); B = std::move(d); }
		else { al_nomem_flag() = false; fprintf(stderr, "[airlift] merge: no usable device, or no device memory for the merge's buffers; the host twin merges the records\n"); }
	}
	if (!B) B.reset(new AlMergeHostBackend(n_threads));
	*backend = D ? "k_merge" : "host twin";
	FILE *fo = fopen(bam_out, "wb");
	if (!fo) { fprintf(stderr, "[ERROR] failed to write the output to file '%s'\n", bam_out); return -1; }
	int rc = -1;
	{
		AlBgzf z(fo, (level & 0xff) | (gpu_deflate && D ? 0x100 : 0), n_threads, D ? D->device : -1);
		const size_t CH = (size_t)al_env().out_piece_mb << 20; char *ring[2] = {nullptr, nullptr};
		bool ok = true;
		if (z.dev_on) for (int i = 0; i < 2; ++i) if (hipHostMalloc((void **)&ring[i], CH, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); ring[i] = nullptr; ok = false; }
		if (!ok) fprintf(stderr, "[ERROR] airlift: merge: no page-locked memory for the BAM output\n");
		if (ok && z.write((const char *)MH.out.data(), MH.out.size()) == 0) {
			AlMergeIn in[AL_MERGE_MAX_IN]; std::vector<std::unique_ptr<AlMergeBgzfSource>> src; bool opened = true;
			for (int i = 0; i < n_in && opened; ++i) {
				in[i].port.B = B.get(); in[i].port.i = i; in[i].fn = bam_in[i]; in[i].start = start[(size_t)i]; in[i].base = out_off[(size_t)i];
				src.emplace_back(new AlMergeBgzfSource()); AlMergeBgzfSource &s = *src.back();
				s.fd = F.fd[(size_t)i]; s.B = &in[i].port; s.fn = bam_in[i];
				if (s.open(zpiece, file_off[(size_t)i], out_off[(size_t)i])) { opened = false; break; }
				s.max_in = zcap; s.max_mem = zmem; in[i].src = &s;
				if (B->set_map(i, MH.map[(size_t)i].data(), (uint32_t)H[(size_t)i].name.size())) opened = false;
			}
			if (opened)
				rc = al_merge_stream(*B, in, n_in, piece_bytes, !z.dev_on, [&](int slot, const AlMergeRound &r) -> int {
					const uint8_t *packed = nullptr;
					if (B->finish(slot, &packed)) return -1;
					if (z.dev_on) {
						const int wd = z.write_device((const char *)D->packed[slot].p, (size_t)r.bytes, D->Cp, ring, CH, D->S[0].ev_out);
						if (wd < 0) return -1;
						if (wd > 0 && (D->fetch_packed(slot, r, &packed) || z.write((const char *)packed, (size_t)r.bytes))) return -1;
					} else if (z.write((const char *)packed, (size_t)r.bytes)) { fprintf(stderr, "[ERROR] failed to write the output to file '%s'\n", bam_out); return -1; }
					return 0;
				}, run);
			src.clear();                                                    // (the sources' page-locked windows go back through the backend)
			if (rc == 0 && z.finish()) { fprintf(stderr, "[ERROR] failed to write the output to file '%s'\n", bam_out); rc = -1; }
		} else if (ok) fprintf(stderr, "[ERROR] failed to write the output to file '%s'\n", bam_out);
		*deflate_s = z.t_deflate;
		if (rc == 0 && z.dev_on && al_env().timing) z.timing_line(stderr, "merge");
		for (int i = 0; i < 2; ++i) if (ring[i]) (void)hipHostFree(ring[i]);
	}                                                                   // (the compressor's device ranges go back before the backend's account is read)
	B->stat(run);
	B.reset();                                                          // every device range goes back here
	if (fclose(fo) == EOF && rc == 0) rc = -1;
	if (rc) unlink(bam_out);
	if (rc == -1 && D && al_nomem_flag()) { al_nomem_flag() = false; *nomem = true; }
	return rc;
}

} // namespace

extern "C" uint32_t al_dbg_merge_tile(void) { return AL_MERGE_TILE; }

extern "C" int al_merge_bams(const char *const *bam_in, int n_in, const char *bam_out, unsigned flags, int device, int n_threads, int level, size_t piece_bytes, AlMergeStat *stat)
{
	const auto t_wall = std::chrono::steady_clock::now();
	if (stat) memset(stat, 0, sizeof(*stat));
	if (n_in < 2 || n_in > AL_MERGE_MAX_IN) { fprintf(stderr, "[ERROR] airlift: merge takes 2 to %d inputs, not %d\n", AL_MERGE_MAX_IN, n_in); return -1; }
	for (int i = 0; i < n_in; ++i) if (!strcmp(bam_in[i], bam_out)) { fprintf(stderr, "[ERROR] airlift: merge: the input '%s' is also the output\n", bam_in[i]); return -1; }
	MergeFiles F; std::vector<AlLiftHeader> H((size_t)n_in); std::vector<uint64_t> file_off((size_t)n_in), out_off((size_t)n_in), start((size_t)n_in); std::vector<std::string> fn;
	for (int i = 0; i < n_in; ++i) {
		F.fd.push_back(open(bam_in[i], O_RDONLY)); fn.push_back(bam_in[i]);
		if (F.fd.back() < 0) { fprintf(stderr, "ERROR: failed to open file '%s'\n", bam_in[i]); return -1; }
		if (const int rc = lift_read_header(F.fd.back(), bam_in[i], H[(size_t)i], &file_off[(size_t)i], &out_off[(size_t)i], &start[(size_t)i], "merge")) return rc;
	}
	AlMergeHeaders MH; std::string err;
	if (al_merge_headers(H, fn, MH, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return -2; }
	const bool host_backend = (flags & AL_MERGE_HOST) != 0, gpu_deflate = (flags & AL_MERGE_GPU_DEFLATE) != 0 && !host_backend;
	std::atomic<size_t> acct{0}; AlMergeRun run; const char *backend = ""; double deflate_s = 0; bool nomem = false;
	int rc = merge_once(bam_in, n_in, F, H, MH, file_off, out_off, start, bam_out, host_backend, gpu_deflate, device, n_threads, level, piece_bytes, run, &backend, &deflate_s, acct, &nomem);
	if (rc && nomem) {
		fprintf(stderr, "[airlift] merge: the device refused memory during the merge; the host twin merges the records from the start\n");
		run = AlMergeRun();
		rc = merge_once(bam_in, n_in, F, H, MH, file_off, out_off, start, bam_out, true, false, device, n_threads, level, piece_bytes, run, &backend, &deflate_s, acct, &nomem);
	}
	const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_wall).count();
	if (stat) {
		stat->n_in = (uint64_t)n_in; stat->records = run.records; stat->rounds = run.rounds; stat->refills = run.refills; stat->bytes_in = run.bytes_in; stat->held = acct.load();
		for (int i = 0; i < n_in; ++i) stat->records_in[i] = run.recs[i];
		stat->read_s = run.read_s; stat->up_s = run.up_s; stat->inflate_s = run.inflate_s; stat->walk_s = run.walk_s; stat->key_s = run.key_s; stat->merge_s = run.merge_s; stat->gather_s = run.gather_s;
		stat->down_s = run.down_s; stat->deflate_s = deflate_s; stat->wall_s = wall; stat->on_device = strcmp(backend, "host twin") != 0;
	}
	if (rc == 0 && al_env().timing) {
		std::string per;
		for (int i = 0; i < n_in; ++i) per += (i ? " + " : "") + std::to_string(run.recs[i]);
		fprintf(stderr, "[airlift] merge: %d inputs into '%s' (%s): %s records, %llu rounds, %llu refills, %llu bytes in; file read %.3f s, copy up %.3f s, inflate %.3f s, walk %.3f s, keys %.3f s, bounds and merge %.3f s, gather %.3f s, copy down %.3f s, deflate %.3f s, wall %.3f s; device bytes held at return: %zu\n",
		        n_in, bam_out, backend, per.c_str(), (unsigned long long)run.rounds, (unsigned long long)run.refills, (unsigned long long)run.bytes_in,
		        run.read_s, run.up_s, run.inflate_s, run.walk_s, run.key_s, run.merge_s, run.gather_s, run.down_s, deflate_s, wall, acct.load());
	}
	if (rc == 0 && (flags & AL_MERGE_WRITE_INDEX)) {                    // the output is closed: the bam-index function over it, with the backend that merged
		rc = al_bai_index_file(bam_out, nullptr, strcmp(backend, "host twin") == 0, device, n_threads, piece_bytes, nullptr, nullptr, nullptr);
		if (rc) fprintf(stderr, "[airlift] merge: '%s' is written, its index is not\n", bam_out);
	}
	return rc;
}

// ---- test taps (airlift_amd/capi.py): al_merge_tap of al_merge.h with the twin and with the kernels ------------------------------------------------------------------
extern "C" int al_dbg_merge_host(const void *const *bam, const size_t *n, int k, size_t piece, uint32_t *tags, uint64_t *keys, size_t rec_cap, size_t *n_out, void *packed, size_t packed_cap, size_t *packed_n, uint64_t *rounds)
{
	AlMergeHostBackend B;
	return al_merge_tap(B, bam, n, k, piece, tags, keys, rec_cap, n_out, packed, packed_cap, packed_n, rounds);
}
extern "C" int al_dbg_merge(int device, const void *const *bam, const size_t *n, int k, size_t piece, uint32_t *tags, uint64_t *keys, size_t rec_cap, size_t *n_out, void *packed, size_t packed_cap, size_t *packed_n, uint64_t *rounds,
                            size_t *held)
{
	*held = 0; *n_out = 0; *packed_n = 0;
	if (k < 2 || k > AL_MERGE_MAX_IN) return -4;
	for (int i = 0; i < k; ++i) if (n[i] >= ((size_t)1 << 31) - 65536) return -3;
	std::atomic<size_t> acct{0}; int rc;
	{
		AlMergeDevBackend B; B.acct = &acct;
		if (B.open(device, k, 0, 0)) return -1;
		rc = al_merge_tap(B, bam, n, k, piece, tags, keys, rec_cap, n_out, packed, packed_cap, packed_n, rounds);
	}
	*held = acct.load();
	return rc;
}

// al_lift.hip -- `lift`: the constant-region reads of a BAM moved across the chain file on the GPU (the function: al_dev_lift.h; the driver: al_lift.h).
//
//   k_bam_walk      one wavefront per text: the record offsets along the chain of block_size fields.  The 64 lanes stage the text in windows of AL_LIFT_W
//                   bytes into LDS with 16-byte loads; the hop through the window is uniform (two LDS words broadcast to every lane, the size field made
//                   scalar) and runs while the next window is already on its way in registers.  The two windows form a ring, so a block_size field cut
//                   by a window's edge is read once the next window is in; a record that ends beyond the next window is skipped by arithmetic and the
//                   window it ends in is loaded afresh.  Lane i & 63 keeps the offset of record i: 64 offsets leave with one store.
//   k_lift          lane per record: the fixed fields and the CIGAR read byte-wise (records are not aligned), at most two binary searches in the block
//                   table, the kept record patched in place; verdict, kept length, arena share
//   (scan)          al_stream_scan_excl_u64 over the kept lengths and over the arena shares
//   k_lift_gather   16 lanes per record: a kept record to the packed output, an unlifted record's descriptor, name and CIGAR words to the arena
// lift --sorted only (the function: ORDER in al_dev_lift.h); without the flag none of these is launched:
//   k_lift_flag          lane per record: 1 for a kept record (verdict KEPT or UNMAPPED), the scan's input
//   (scan)               al_stream_scan_excl_u64 over the flags: a kept record's index in the compacted list, and their number
//   k_lift_compact       lane per record: (key, record index) of a kept record to its compacted index
//   k_lift_descents      lane per compacted index: key[i] < key[i - 1] counted per wavefront, one atomic per wavefront; the count comes down with run()'s counts
//   (sort)               rocprim::radix_sort_pairs (stable) through al_prim_run, only when the piece has a descent
//   k_lift_plen          lane per compacted index: the length of the record that leaves at that index; then the scan over them
//   k_lift_gather_sorted 16 lanes per record: the unlifted records to the arena as k_lift_gather does, then kept record perm[i] to off[i]
// A backend slot is an input-only AlStreamSlot (text, stream, inflater staging), as in al_select.hip.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <atomic>
#include <memory>
#include "al_internal.h"
#include "al_device.h"
#include "al_runtime.h"
#include "al_stream.h"
#include "al_dev_inflate.h"
#include "al_bam.h"
#include "al_lift.h"
#include "al_dev_walk.h"
#include "al_run_store.h"
#include "al_bai.h"
#include "al_prim.h"
#include "../../include/airlift.h"

__global__ void __launch_bounds__(256)
k_lift(uint8_t *__restrict__ t, const uint32_t *__restrict__ rec_off, uint32_t n_rec, AlLiftTab T, uint32_t *__restrict__ verdict, uint32_t *__restrict__ keep_len, uint32_t *__restrict__ arena_len,
       unsigned long long *__restrict__ first_bad, unsigned long long *__restrict__ cnt)
{
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t v = 0xffu;
	if (r < n_rec) {
		const AlLiftOut o = al_lift_record(T, t + rec_off[r]);
		verdict[r] = v = o.verdict; keep_len[r] = o.keep_len; arena_len[r] = o.arena_len;
		if (v >= AL_LIFT_BAD_FIT) atomicMin(first_bad, (unsigned long long)r);
	} else if (r == n_rec) { keep_len[r] = 0; arena_len[r] = 0; }          // (the scans' last element: their totals)
	for (uint32_t c = 0; c < 3; ++c) {
		const unsigned long long m = __ballot(v == c);
		if ((threadIdx.x & 63) == 0 && m) atomicAdd(cnt + c, (unsigned long long)__popcll(m));
	}
}

__global__ void __launch_bounds__(256)
k_lift_gather(const uint8_t *__restrict__ t, const uint32_t *__restrict__ rec_off, uint32_t n_rec, const uint32_t *__restrict__ verdict, const uint32_t *__restrict__ keep_len,
              const uint64_t *__restrict__ keep_off, const uint64_t *__restrict__ arena_off, uint8_t *__restrict__ packed, uint8_t *__restrict__ arena)
{
	const uint32_t r = blockIdx.x * 16 + (threadIdx.x >> 4), l = threadIdx.x & 15;
	if (r >= n_rec) return;
	const uint8_t *src = t + rec_off[r];
	const uint32_t v = verdict[r];
	if (v == AL_LIFT_UNLIFTED) al_lift_arena_put(src, arena + arena_off[r], l, 16);
	else if (v == AL_LIFT_KEPT || v == AL_LIFT_UNMAPPED) {
		const uint32_t len = keep_len[r];
		uint8_t *o = packed + keep_off[r];
		for (uint32_t j = l; j < len; j += 16) o[j] = src[j];
	}
}

// ---- lift --sorted ---------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_lift_flag(const uint32_t *__restrict__ verdict, uint32_t n_rec, uint32_t *__restrict__ flag)
{
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r < n_rec) { const uint32_t v = verdict[r]; flag[r] = v == AL_LIFT_KEPT || v == AL_LIFT_UNMAPPED ? 1u : 0u; }
	else if (r == n_rec) flag[r] = 0;                                       // (the scan's last element: the number of kept records)
}
__global__ void __launch_bounds__(256)
k_lift_compact(const uint8_t *__restrict__ t, const uint32_t *__restrict__ rec_off, uint32_t n_rec, const uint32_t *__restrict__ flag, const uint64_t *__restrict__ idx,
               uint64_t *__restrict__ key, uint32_t *__restrict__ ridx)
{
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n_rec || !flag[r]) return;
	const uint64_t i = idx[r];                                              // (< the number of kept records <= n_rec: the arrays hold n_rec + 2)
	key[i] = al_lift_key(t + rec_off[r]); ridx[i] = r;
}
// n_kept: on the device (the scan's total); the grid covers n_rec, an upper bound of it
__global__ void __launch_bounds__(256)
k_lift_descents(const uint64_t *__restrict__ key, const uint64_t *__restrict__ n_kept, unsigned long long *__restrict__ cnt)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, n = *n_kept;
	const bool d = i > 0 && i < n && key[i] < key[i - 1];
	const unsigned long long m = __ballot(d);
	if ((threadIdx.x & 63) == 0 && m) atomicAdd(cnt, (unsigned long long)__popcll(m));
}
__global__ void __launch_bounds__(256)
k_lift_plen(const uint32_t *__restrict__ keep_len, const uint32_t *__restrict__ perm, uint32_t n_kept, uint32_t *__restrict__ plen)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n_kept) plen[i] = keep_len[perm[i]];
	else if (i == n_kept) plen[i] = 0;
}
// groups [0, n_rec): record r, when it is unlifted, to the arena; groups [n_rec, n_rec + n_kept): the kept record perm[i] to packed + off[i]
__global__ void __launch_bounds__(256)
k_lift_gather_sorted(const uint8_t *__restrict__ t, const uint32_t *__restrict__ rec_off, uint32_t n_rec, const uint32_t *__restrict__ verdict, const uint64_t *__restrict__ arena_off, uint8_t *__restrict__ arena,
                     const uint32_t *__restrict__ perm, uint32_t n_kept, const uint32_t *__restrict__ plen, const uint64_t *__restrict__ off, uint8_t *__restrict__ packed)
{
	const uint32_t g = blockIdx.x * 16 + (threadIdx.x >> 4), l = threadIdx.x & 15;
	if (g < n_rec) { if (verdict[g] == AL_LIFT_UNLIFTED) al_lift_arena_put(t + rec_off[g], arena + arena_off[g], l, 16); return; }
	const uint32_t i = g - n_rec;
	if (i >= n_kept) return;
	const uint8_t *src = t + rec_off[perm[i]];
	const uint32_t len = plen[i];
	uint8_t *o = packed + off[i];
	for (uint32_t j = l; j < len; j += 16) o[j] = src[j];
}

namespace {

#define LIFT_CHECK(x) AL_HIP_CHECK_AS("lift", x)

struct AlLiftDevBackend : AlLiftBackend {
	int device = 0; bool open_ok = false;
	std::atomic<size_t> own_acct{0}, *acct = &own_acct, *acct_before = nullptr;     // the account every device range of the backend is booked on
	AlStreamSlot S[2];
	AlLiftBlock *d_blk = nullptr; uint32_t *d_pmax = nullptr, *d_first = nullptr; int32_t *d_ref = nullptr; AlLiftTab T{nullptr, nullptr, nullptr, nullptr, 0, 0};
	DevBuf<uint32_t> rec_off[2], verdict[2], keep_len[2], arena_len[2]; DevBuf<uint64_t> keep_off[2], arena_off[2]; DevBuf<uint8_t> packed[2], arena[2];
	DevBuf<unsigned long long> cnt[2];                                  // first_bad, kept, unlifted, unmapped; the walk's three words behind them
	PinnedVec<uint8_t> h_packed[2], h_arena[2];
	unsigned long long *h_cnt = nullptr;                                // page-locked, 16 words per slot
	hipEvent_t ev[2][6] = {};                                          // per slot: walk from / to, lift to, gather from / to, copy down to
	bool gathered[2] = {false, false}; uint32_t n_rec[2] = {0, 0};
	double up_s = 0, walk_s = 0, lift_s = 0, down_s = 0;
	// lift --sorted: the kept flags and their scan, the compacted (key, record index) pairs and the sort's outputs and temporaries, lengths and offsets in packed order
	DevBuf<uint32_t> kflag[2], ridx[2], ridx2[2], plen[2]; DevBuf<uint64_t> kidx[2], key[2], key2[2], poff[2]; DevBuf<uint8_t> sort_tmp[2];
	PinnedVec<uint64_t> h_key[2]; PinnedVec<uint32_t> h_len[2];
	const uint64_t *key_s[2] = {nullptr, nullptr}; const uint32_t *ridx_s[2] = {nullptr, nullptr};   // the pairs in packed order: key / ridx, or key2 / ridx2 after a sort
	hipEvent_t ev_sort[2][2] = {};
	bool did_sort[2] = {false, false}, refuse_tmp = false, noticed = false; size_t n_packed[2] = {0, 0};   // refuse_tmp (the taps): the sort's temporaries count as refused
	double sort_s = 0, sgather_s = 0;

	const char *name() const override { return "k_lift"; }
	// 0, or 1 when there is no usable device or it refuses the memory (nothing is left allocated after the destructor)
	int open(int dev, const AlLiftChain &C, size_t piece, size_t cap_in, size_t cap_mem)
	{
		int n_dev = 0;
		if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) { (void)hipGetLastError(); return 1; }
		device = dev < 0 ? 0 : dev;
		if (device >= n_dev || hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return 1; }
		acct_before = al_acct(); al_acct() = acct; open_ok = true;
		for (int i = 0; i < 2; ++i) {
			if (al_stream_slot_init(S[i], nullptr, device, 1)) return 1;
			for (hipEvent_t &e : ev[i]) if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); return 1; }
			for (hipEvent_t &e : ev_sort[i]) if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); return 1; }
			if (al_stream_begin_text(S[i], 0, 2 * piece + 65536) || cnt[i].ensure(8)) return 1;
			if (cap_in && al_stream_bgzf_init(S[i], cap_in, cap_mem)) return 1;
		}
		if (hipHostMalloc((void **)&h_cnt, 32 * 8, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); h_cnt = nullptr; return 1; }
		const size_t nb = C.blk.size(), nr = C.ref_slot.size();
		if (al_dev_malloc((void **)&d_blk, (nb + 1) * sizeof(AlLiftBlock)) != hipSuccess || al_dev_malloc((void **)&d_pmax, (nb + 1) * 4) != hipSuccess ||
		    al_dev_malloc((void **)&d_first, C.first.size() * 4) != hipSuccess || al_dev_malloc((void **)&d_ref, (nr + 1) * 4) != hipSuccess) { (void)hipGetLastError(); return 1; }
		if ((nb && (hipMemcpy(d_blk, C.blk.data(), nb * sizeof(AlLiftBlock), hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_pmax, C.pmax.data(), nb * 4, hipMemcpyHostToDevice) != hipSuccess)) ||
		    hipMemcpy(d_first, C.first.data(), C.first.size() * 4, hipMemcpyHostToDevice) != hipSuccess || (nr && hipMemcpy(d_ref, C.ref_slot.data(), nr * 4, hipMemcpyHostToDevice) != hipSuccess)) { (void)hipGetLastError(); return 1; }
		T = AlLiftTab{d_blk, d_pmax, d_first, d_ref, (uint32_t)C.tname.size(), (uint32_t)nr};
		return 0;
	}
	~AlLiftDevBackend() override
	{
		if (!open_ok) return;
		(void)hipSetDevice(device);
		for (int i = 0; i < 2; ++i) {
			if (S[i].io) (void)hipStreamSynchronize(S[i].io);
			rec_off[i].release(); verdict[i].release(); keep_len[i].release(); arena_len[i].release(); keep_off[i].release(); arena_off[i].release(); packed[i].release(); arena[i].release(); cnt[i].release();
			kflag[i].release(); ridx[i].release(); ridx2[i].release(); plen[i].release(); kidx[i].release(); key[i].release(); key2[i].release(); poff[i].release(); sort_tmp[i].release();
			al_stream_slot_destroy(S[i]);
			for (hipEvent_t &e : ev[i]) if (e) (void)hipEventDestroy(e);
			for (hipEvent_t &e : ev_sort[i]) if (e) (void)hipEventDestroy(e);
		}
		if (d_blk) al_dev_free(d_blk); if (d_pmax) al_dev_free(d_pmax); if (d_first) al_dev_free(d_first); if (d_ref) al_dev_free(d_ref);
		if (h_cnt) (void)hipHostFree(h_cnt);
		al_acct() = acct_before;
	}
	size_t held() const override { return acct->load(); }

	int begin(int s, size_t cap) override { if (al_stream_begin_text(S[s], 0, cap + 2 * AL_LIFT_W)) return -1; gathered[s] = false; return 0; }   // (room for k_bam_walk to load whole windows)
	int room(int s, uint64_t n) const { if (S[s].txt_n[0] + n + 16 > S[s].txt[0].cap) { fprintf(stderr, "[airlift] lift: text buffer too small\n"); return -1; } return 0; }
	int carry(int s, int from, uint64_t off, uint64_t n) override
	{
		if (n == 0) return 0;
		if (room(s, n) || off + n > S[from].txt_n[0]) return -1;
		LIFT_CHECK(hipMemcpyAsync(S[s].txt[0].p + S[s].txt_n[0], S[from].txt[0].p + off, n, hipMemcpyDeviceToDevice, S[s].io));
		S[s].txt_n[0] += n;
		return 0;
	}
	int append(int s, const uint8_t *p, size_t n) override
	{
		if (n == 0) return 0;
		if (room(s, n)) return -1;
		LIFT_CHECK(hipMemcpyAsync(S[s].txt[0].p + S[s].txt_n[0], p, n, hipMemcpyHostToDevice, S[s].io));
		LIFT_CHECK(hipStreamSynchronize(S[s].io));
		S[s].txt_n[0] += n;
		return 0;
	}
	int append_bgzf(int s, const uint8_t *b, size_t n_in, const AlInfMember *mem, size_t n_mem, uint64_t n_out, size_t *bad, uint32_t *bad_status) override
	{
		const auto t0 = std::chrono::steady_clock::now(); const double k0 = S[s].bz.kernel_s;
		const int r = al_stream_append_bgzf(S[s], 0, b, n_in, mem, n_mem, n_out, bad, bad_status);
		up_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() - (S[s].bz.kernel_s - k0);
		return r;
	}
	uint64_t text_bytes(int s) const override { return S[s].txt_n[0]; }
	int run(int s, uint64_t start, AlLiftPiece *r) override
	{
		AlStreamSlot &X = S[s]; hipStream_t st = X.io;
		LIFT_CHECK(hipSetDevice(device));
		*r = AlLiftPiece();
		const uint64_t n = X.txt_n[0];
		if (n >= (1ull << 31) || start > n) { fprintf(stderr, "[airlift] lift: a text of %llu bytes\n", (unsigned long long)n); return -1; }
		const size_t cap = (size_t)(n / 36) + 64;                       // (a record takes at least 36 bytes)
		if (rec_off[s].ensure(cap)) return -1;
		unsigned long long *h = h_cnt + 16 * s; uint32_t *hw = (uint32_t *)(h + 4);
		h[0] = ~0ull; h[1] = h[2] = h[3] = 0;
		LIFT_CHECK(hipMemcpyAsync(cnt[s].p, h, 32, hipMemcpyHostToDevice, st));
		LIFT_CHECK(hipEventRecord(ev[s][0], st));
		hipLaunchKernelGGL(k_bam_walk, dim3(1), dim3(64), 0, st, X.txt[0].p, (uint32_t)n, (uint32_t)std::min<size_t>(X.txt[0].cap, 0xfffffff0u), (uint32_t)start, rec_off[s].p, (uint32_t *)(cnt[s].p + 4));
		LIFT_CHECK(hipEventRecord(ev[s][1], st));
		LIFT_CHECK(hipMemcpyAsync(hw, cnt[s].p + 4, 12, hipMemcpyDeviceToHost, st));
		LIFT_CHECK(hipStreamSynchronize(st));
		LIFT_CHECK(hipGetLastError());
		const uint32_t nr = hw[0];
		r->n_rec = nr; r->consumed = hw[1]; r->walk_bad = hw[2]; n_rec[s] = nr;
		if (verdict[s].ensure((size_t)nr + 2) || keep_len[s].ensure((size_t)nr + 2) || arena_len[s].ensure((size_t)nr + 2) || keep_off[s].ensure((size_t)nr + 2) || arena_off[s].ensure((size_t)nr + 2)) return -1;
		hipLaunchKernelGGL(k_lift, dim3((nr + 256) / 256), dim3(256), 0, st, X.txt[0].p, rec_off[s].p, nr, T, verdict[s].p, keep_len[s].p, arena_len[s].p, cnt[s].p, cnt[s].p + 1);
		if (al_stream_scan_excl_u64(X, keep_len[s].p, keep_off[s].p, (size_t)nr + 1, st) || al_stream_scan_excl_u64(X, arena_len[s].p, arena_off[s].p, (size_t)nr + 1, st)) return -1;
		if (sorted) {                                                   // the compacted (key, record index) pairs and their descents; the count comes down with the others
			if (kflag[s].ensure((size_t)nr + 2) || kidx[s].ensure((size_t)nr + 2) || key[s].ensure((size_t)nr + 2) || ridx[s].ensure((size_t)nr + 2)) return -1;
			LIFT_CHECK(hipMemsetAsync(cnt[s].p + 6, 0, 8, st));
			hipLaunchKernelGGL(k_lift_flag, dim3((nr + 256) / 256), dim3(256), 0, st, verdict[s].p, nr, kflag[s].p);
			if (al_stream_scan_excl_u64(X, kflag[s].p, kidx[s].p, (size_t)nr + 1, st)) return -1;
			if (nr) {
				hipLaunchKernelGGL(k_lift_compact, dim3((nr + 255) / 256), dim3(256), 0, st, X.txt[0].p, rec_off[s].p, nr, kflag[s].p, kidx[s].p, key[s].p, ridx[s].p);
				hipLaunchKernelGGL(k_lift_descents, dim3((nr + 255) / 256), dim3(256), 0, st, key[s].p, kidx[s].p + nr, cnt[s].p + 6);
			}
			LIFT_CHECK(hipMemcpyAsync(h + 8, cnt[s].p + 6, 8, hipMemcpyDeviceToHost, st));
		}
		LIFT_CHECK(hipEventRecord(ev[s][2], st));
		LIFT_CHECK(hipMemcpyAsync(h, cnt[s].p, 32, hipMemcpyDeviceToHost, st));
		LIFT_CHECK(hipMemcpyAsync(h + 6, keep_off[s].p + nr, 8, hipMemcpyDeviceToHost, st));
		LIFT_CHECK(hipMemcpyAsync(h + 7, arena_off[s].p + nr, 8, hipMemcpyDeviceToHost, st));
		LIFT_CHECK(hipStreamSynchronize(st));
		LIFT_CHECK(hipGetLastError());
		r->first_bad = h[0]; r->n_kept = h[1]; r->n_unlifted = h[2]; r->n_unmapped = h[3]; r->kept_bytes = h[6]; r->arena_bytes = h[7];
		if (sorted) r->descents = h[8];
		if (r->first_bad != ~0ull) {
			uint32_t two[2] = {0, 0};
			LIFT_CHECK(hipMemcpy(&two[0], rec_off[s].p + r->first_bad, 4, hipMemcpyDeviceToHost)); LIFT_CHECK(hipMemcpy(&two[1], verdict[s].p + r->first_bad, 4, hipMemcpyDeviceToHost));
			r->bad_off = two[0]; r->bad_code = two[1];
		}
		float ms[2] = {0, 0};
		if (hipEventElapsedTime(&ms[0], ev[s][0], ev[s][1]) == hipSuccess && hipEventElapsedTime(&ms[1], ev[s][1], ev[s][2]) == hipSuccess) { walk_s += ms[0] * 1e-3; lift_s += ms[1] * 1e-3; } else (void)hipGetLastError();
		return 0;
	}
	int gather(int s, const AlLiftPiece &r, bool packed_down) override
	{
		AlStreamSlot &X = S[s]; hipStream_t st = X.io;
		if (packed[s].ensure((size_t)r.kept_bytes + 16) || arena[s].ensure((size_t)r.arena_bytes + 16) || h_arena[s].resize((size_t)r.arena_bytes + 1) || (packed_down && h_packed[s].resize((size_t)r.kept_bytes + 1))) return -1;
		if (sorted) return gather_sorted(s, r);
		LIFT_CHECK(hipEventRecord(ev[s][3], st));
		if (r.n_rec) hipLaunchKernelGGL(k_lift_gather, dim3((unsigned)((r.n_rec + 15) / 16)), dim3(256), 0, st, X.txt[0].p, rec_off[s].p, (uint32_t)r.n_rec, verdict[s].p, keep_len[s].p, keep_off[s].p, arena_off[s].p, packed[s].p, arena[s].p);
		LIFT_CHECK(hipEventRecord(ev[s][4], st));
		if (r.arena_bytes) LIFT_CHECK(hipMemcpyAsync(h_arena[s].data(), arena[s].p, (size_t)r.arena_bytes, hipMemcpyDeviceToHost, st));
		if (packed_down && r.kept_bytes) LIFT_CHECK(hipMemcpyAsync(h_packed[s].data(), packed[s].p, (size_t)r.kept_bytes, hipMemcpyDeviceToHost, st));
		LIFT_CHECK(hipEventRecord(ev[s][5], st));
		LIFT_CHECK(hipGetLastError());
		gathered[s] = true;
		return 0;
	}
	// lift --sorted: the pairs sorted when the piece has a descent, the kept records packed in that order, their keys and lengths brought down beside the bytes
	int gather_sorted(int s, const AlLiftPiece &r)
	{
		AlStreamSlot &X = S[s]; hipStream_t st = X.io;
		const size_t nk = (size_t)r.n_packed(); const uint32_t nr = (uint32_t)r.n_rec;
		if (h_packed[s].resize((size_t)r.kept_bytes + 1)) return -1;
		n_packed[s] = nk; did_sort[s] = false; key_s[s] = key[s].p; ridx_s[s] = ridx[s].p;
		if (plen[s].ensure(nk + 2) || poff[s].ensure(nk + 2) || h_key[s].resize(nk + 1) || h_len[s].resize(nk + 1)) return -1;
		if (r.descents) {
			if (key2[s].ensure(nk + 2) || ridx2[s].ensure(nk + 2)) return -1;
			LIFT_CHECK(hipEventRecord(ev_sort[s][0], st));
			const int sr = refuse_tmp ? AL_ERR_NOMEM : al_prim_run(sort_tmp[s], [&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, (const uint64_t *)key[s].p, key2[s].p, (const uint32_t *)ridx[s].p, ridx2[s].p, nk, 0, 64, st); }, "lift");
			if (sr == AL_ERR_NOMEM) {                                        // the temporaries are refused: this piece's order is made on the host from the keys
				al_nomem_flag() = false;
				if (!noticed) { fprintf(stderr, "[airlift] lift --sorted: no device memory for the sort's temporaries; the keys of such a piece are sorted on the host\n"); noticed = true; }
				std::vector<uint64_t> k(nk), k2(nk); std::vector<uint32_t> x(nk), x2(nk), perm(nk);
				LIFT_CHECK(hipMemcpyAsync(k.data(), key[s].p, nk * 8, hipMemcpyDeviceToHost, st)); LIFT_CHECK(hipMemcpyAsync(x.data(), ridx[s].p, nk * 4, hipMemcpyDeviceToHost, st));
				LIFT_CHECK(hipStreamSynchronize(st));
				for (size_t i = 0; i < nk; ++i) perm[i] = (uint32_t)i;
				std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return k[a] < k[b]; });
				for (size_t i = 0; i < nk; ++i) { k2[i] = k[perm[i]]; x2[i] = x[perm[i]]; }
				LIFT_CHECK(hipMemcpyAsync(key2[s].p, k2.data(), nk * 8, hipMemcpyHostToDevice, st)); LIFT_CHECK(hipMemcpyAsync(ridx2[s].p, x2.data(), nk * 4, hipMemcpyHostToDevice, st));
				LIFT_CHECK(hipStreamSynchronize(st));                           // (the vectors go out of scope)
			} else if (sr) return -1;
			else did_sort[s] = true;
			LIFT_CHECK(hipEventRecord(ev_sort[s][1], st));
			key_s[s] = key2[s].p; ridx_s[s] = ridx2[s].p;
		}
		LIFT_CHECK(hipEventRecord(ev[s][3], st));
		hipLaunchKernelGGL(k_lift_plen, dim3((unsigned)((nk + 256) / 256)), dim3(256), 0, st, keep_len[s].p, ridx_s[s], (uint32_t)nk, plen[s].p);
		if (al_stream_scan_excl_u64(X, plen[s].p, poff[s].p, nk + 1, st)) return -1;
		if (nr + nk) hipLaunchKernelGGL(k_lift_gather_sorted, dim3((unsigned)(((size_t)nr + nk + 15) / 16)), dim3(256), 0, st, X.txt[0].p, rec_off[s].p, nr, verdict[s].p, arena_off[s].p, arena[s].p,
		                                ridx_s[s], (uint32_t)nk, plen[s].p, poff[s].p, packed[s].p);
		LIFT_CHECK(hipEventRecord(ev[s][4], st));
		if (r.arena_bytes) LIFT_CHECK(hipMemcpyAsync(h_arena[s].data(), arena[s].p, (size_t)r.arena_bytes, hipMemcpyDeviceToHost, st));
		if (r.kept_bytes) LIFT_CHECK(hipMemcpyAsync(h_packed[s].data(), packed[s].p, (size_t)r.kept_bytes, hipMemcpyDeviceToHost, st));
		if (nk) { LIFT_CHECK(hipMemcpyAsync(h_key[s].data(), key_s[s], nk * 8, hipMemcpyDeviceToHost, st)); LIFT_CHECK(hipMemcpyAsync(h_len[s].data(), plen[s].p, nk * 4, hipMemcpyDeviceToHost, st)); }
		LIFT_CHECK(hipEventRecord(ev[s][5], st));
		LIFT_CHECK(hipGetLastError());
		gathered[s] = true;
		return 0;
	}
	int sorted_out(int s, const uint64_t **k, const uint32_t **l) override { *k = h_key[s].data(); *l = h_len[s].data(); return 0; }
	int fetch_perm(int s, uint32_t *perm, size_t n) override { if (n > n_packed[s]) return -1; if (n) LIFT_CHECK(hipMemcpy(perm, ridx_s[s], n * 4, hipMemcpyDeviceToHost)); return 0; }
	bool sort_launched(int s) const override { return did_sort[s]; }
	int finish(int s, const uint8_t **p, const uint8_t **a) override
	{
		LIFT_CHECK(hipStreamSynchronize(S[s].io));
		LIFT_CHECK(hipGetLastError());
		*p = h_packed[s].data(); *a = h_arena[s].data();
		if (gathered[s]) {
			float ms[2] = {0, 0};
			if (hipEventElapsedTime(&ms[0], ev[s][3], ev[s][4]) == hipSuccess && hipEventElapsedTime(&ms[1], ev[s][4], ev[s][5]) == hipSuccess) { lift_s += ms[0] * 1e-3; down_s += ms[1] * 1e-3; if (sorted) sgather_s += ms[0] * 1e-3; } else (void)hipGetLastError();
			if (sorted && did_sort[s]) { if (hipEventElapsedTime(&ms[0], ev_sort[s][0], ev_sort[s][1]) == hipSuccess) sort_s += ms[0] * 1e-3; else (void)hipGetLastError(); }
			gathered[s] = false;
		}
		return 0;
	}
	// the packed records of a slot after finish(), for a slot whose bytes did not come down with the gather
	int fetch_packed(int s, const AlLiftPiece &r, const uint8_t **p)
	{
		if (h_packed[s].resize((size_t)r.kept_bytes + 1)) return -1;
		const auto t0 = std::chrono::steady_clock::now();
		if (r.kept_bytes) LIFT_CHECK(hipMemcpy(h_packed[s].data(), packed[s].p, (size_t)r.kept_bytes, hipMemcpyDeviceToHost));
		down_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
		*p = h_packed[s].data();
		return 0;
	}
	void *host_buffer(size_t n) override { void *p = nullptr; if (hipHostMalloc(&p, n, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; } return p; }
	void host_buffer_free(void *p) override { (void)hipHostFree(p); }
	int fetch_records(int s, uint32_t *ro, uint32_t *v, size_t n) override
	{
		if (n) { LIFT_CHECK(hipMemcpy(ro, rec_off[s].p, n * 4, hipMemcpyDeviceToHost)); LIFT_CHECK(hipMemcpy(v, verdict[s].p, n * 4, hipMemcpyDeviceToHost)); }
		return 0;
	}
	void stat(AlLiftRun &st) override { st.up_s += up_s; st.inflate_s += S[0].bz.kernel_s + S[1].bz.kernel_s; st.walk_s += walk_s; st.lift_s += lift_s; st.down_s += down_s; st.sort_s += sort_s; st.sgather_s += sgather_s; }
};

} // namespace

extern "C" uint32_t al_dbg_lift_window(void) { return AL_LIFT_W; }

extern "C" int al_lift_bam(const char *bam_in, const char *chain_fn, const char *bam_out, const char *bed_out, unsigned flags, int device, int n_threads, int level, size_t piece_bytes, AlLiftStat *stat)
{
	const auto t_wall = std::chrono::steady_clock::now();
	const size_t piece_bytes_arg = piece_bytes;
	if (stat) memset(stat, 0, sizeof(*stat));
	if ((flags & AL_LIFT_WRITE_INDEX) && !(flags & AL_LIFT_SORTED)) { fprintf(stderr, "[ERROR] airlift: lift: an index needs a BAM in coordinate order: --write-index goes with --sorted\n"); return -1; }
	AlLiftChain C; std::string err;
	if (al_lift_build(chain_fn, C, err)) { fprintf(stderr, "[ERROR] airlift: %s\n", err.c_str()); return -1; }
	const int fd = open(bam_in, O_RDONLY);
	if (fd < 0) { fprintf(stderr, "ERROR: failed to open file '%s'\n", bam_in); return -1; }
	AlLiftHeader H; uint64_t file_off = 0, out_off = 0, start = 0;
	int rc = lift_read_header(fd, bam_in, H, &file_off, &out_off, &start);
	if (rc == 0 && al_lift_bind(C, H, err)) { fprintf(stderr, "[ERROR] airlift: lift: '%s': %s\n", bam_in, err.c_str()); rc = -1; }
	if (rc) { close(fd); return rc; }
	FILE *fo = fopen(bam_out, "wb"), *fb = fo ? fopen(bed_out, "wb") : nullptr;
	if (!fo || !fb) { fprintf(stderr, "[ERROR] failed to write the output to file '%s'\n", fo ? bed_out : bam_out); if (fo) { fclose(fo); unlink(bam_out); } close(fd); return -1; }
	const bool sorted = (flags & AL_LIFT_SORTED) != 0;
	const bool host_backend = (flags & AL_LIFT_HOST) != 0, gpu_deflate = (flags & AL_LIFT_GPU_DEFLATE) != 0 && !host_backend;
	const size_t zpiece = (size_t)al_env().inflate_piece_kb << 10, zcap = 2 * zpiece + 65536, zmem = zcap / 64 + 1024;
	if (piece_bytes == 0) piece_bytes = std::max((size_t)8 << 20, 4 * zpiece);
	if (piece_bytes >= ((size_t)1 << 29)) piece_bytes = (size_t)1 << 29;
	std::atomic<size_t> acct{0}; AlLiftRun run; const char *backend = ""; double deflate_s = 0, merge_s = 0; uint64_t spills = 0, runs_chained = 0; rc = -1;
	{
		std::unique_ptr<AlLiftBackend> B; AlLiftDevBackend *D = nullptr;
		if (!host_backend) {
			std::unique_ptr<AlLiftDevBackend> d(new AlLiftDevBackend()); d->acct = &acct;
			if (d->open(device, C, piece_bytes, zcap, zmem) == 0) { D = d.get(); B = std::move(d); }
			else fprintf(stderr, "[airlift] lift: no usable device, or no device memory for the lift's buffers; the host twin lifts the reads\n");
		}
		if (!B) B.reset(new AlLiftHostBackend(C.tab(), n_threads));
		backend = B->name();
		B->set_sorted(sorted);
		AlRunStore store; store.limit = (size_t)al_env_sort_mem();      // lift --sorted: the pieces, each in order, until the end of the input
		{
			AlBgzf z(fo, (level & 0xff) | (gpu_deflate && D ? 0x100 : 0), n_threads, D ? D->device : -1);
			const size_t CH = (size_t)al_env().out_piece_mb << 20; char *ring[2] = {nullptr, nullptr};
			bool ok = true;
			if (z.dev_on) for (int i = 0; i < 2; ++i) if (hipHostMalloc((void **)&ring[i], CH, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); ring[i] = nullptr; ok = false; }
			if (!ok) fprintf(stderr, "[ERROR] airlift: lift: no page-locked memory for the BAM output\n");
			std::vector<uint8_t> hdr; al_lift_header_write(H, C, hdr, sorted);
			std::string rows;
			if (ok && z.write((const char *)hdr.data(), hdr.size()) == 0) {
				AlLiftBgzfSource src; src.fd = fd; src.B = B.get(); src.fn = bam_in;
				if (src.open(zpiece, file_off, out_off) == 0) {
					src.max_in = zcap; src.max_mem = zmem;
					rc = al_lift_stream(*B, src, piece_bytes, start, out_off, bam_in, !z.dev_on || sorted, [&](int slot, const AlLiftPiece &r) -> int {
						const uint8_t *packed = nullptr, *arena = nullptr;
						if (B->finish(slot, &packed, &arena)) return -1;
						if (sorted) {
							const uint64_t *keys = nullptr; const uint32_t *lens = nullptr;
							if (B->sorted_out(slot, &keys, &lens)) return -1;
							++(r.descents ? run.sorted_pieces : run.in_order);
							const auto t0 = std::chrono::steady_clock::now();
							const int ar = store.add_run(packed, (size_t)r.kept_bytes, keys, lens, (size_t)r.n_packed());
							merge_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
							if (ar) return -1;
						} else if (z.dev_on) {
							const int wd = z.write_device((const char *)D->packed[slot].p, (size_t)r.kept_bytes, D->S[slot].io, ring, CH, D->S[slot].ev_out);
							if (wd < 0) return -1;
							if (wd > 0 && (D->fetch_packed(slot, r, &packed) || z.write((const char *)packed, (size_t)r.kept_bytes))) return -1;
						} else if (z.write((const char *)packed, (size_t)r.kept_bytes)) { fprintf(stderr, "[ERROR] failed to write the output to file '%s'\n", bam_out); return -1; }
						rows.clear(); al_lift_rows(arena, (size_t)r.arena_bytes, H, rows);
						if (fwrite(rows.data(), 1, rows.size(), fb) != rows.size()) { fprintf(stderr, "[ERROR] failed to write the output to file '%s'\n", bed_out); return -1; }
						return 0;
					}, run);
				}
				if (rc == 0 && sorted) {                                    // the merge: host bytes into the compressor, whichever it is
					const auto t0 = std::chrono::steady_clock::now();
					if (store.finish([&](const uint8_t *p, size_t n) { return z.write((const char *)p, n); })) { fprintf(stderr, "[ERROR] failed to write the output to file '%s'\n", bam_out); rc = -1; }
					merge_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() - store.emit_s;
					spills = store.spills; runs_chained = store.chained;
				}
				if (rc == 0 && z.finish()) { fprintf(stderr, "[ERROR] failed to write the output to file '%s'\n", bam_out); rc = -1; }
			} else if (ok) fprintf(stderr, "[ERROR] failed to write the output to file '%s'\n", bam_out);
			deflate_s = z.t_deflate;
			if (rc == 0 && z.dev_on && al_env().timing) z.timing_line(stderr, "lift");
			for (int i = 0; i < 2; ++i) if (ring[i]) (void)hipHostFree(ring[i]);
		}                                                               // (the compressor's device ranges go back before the backend's account is read)
		B->stat(run);
		B.reset();                                                      // every device range goes back here
	}
	close(fd);
	if (fclose(fo) == EOF && rc == 0) rc = -1;
	if (fclose(fb) == EOF && rc == 0) rc = -1;
	if (rc) { unlink(bam_out); unlink(bed_out); }
	const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_wall).count();
	if (stat) {
		stat->kept = run.kept; stat->unlifted = run.unlifted; stat->unmapped_kept = run.unmapped_kept; stat->pieces = run.pieces; stat->bytes_in = run.bytes_in;
		stat->read_s = run.read_s; stat->up_s = run.up_s; stat->inflate_s = run.inflate_s; stat->walk_s = run.walk_s; stat->lift_s = run.lift_s; stat->down_s = run.down_s; stat->deflate_s = deflate_s; stat->wall_s = wall;
		stat->held = acct.load(); stat->on_device = strcmp(backend, "host twin") != 0;
	}
	if (rc == 0 && al_env().timing)
		fprintf(stderr, "[airlift] lift: '%s' (%s): %llu pieces, %llu bytes in, %llu kept, %llu unlifted, %llu unmapped kept; file read %.3f s, copy up %.3f s, inflate %.3f s, walk %.3f s, lift and gather %.3f s, copy down %.3f s, deflate %.3f s, wall %.3f s; device bytes held at return: %zu\n",
		        bam_in, backend, (unsigned long long)run.pieces, (unsigned long long)run.bytes_in, (unsigned long long)run.kept, (unsigned long long)run.unlifted, (unsigned long long)run.unmapped_kept,
		        run.read_s, run.up_s, run.inflate_s, run.walk_s, run.lift_s, run.down_s, deflate_s, wall, acct.load());
	if (rc == 0 && sorted && al_env().timing)
		fprintf(stderr, "[airlift] lift --sorted: %llu pieces in order, %llu pieces sorted, %llu chained onto the run before, %llu spills; sort %.3f s, permuted gather %.3f s, host merge %.3f s\n",
		        (unsigned long long)run.in_order, (unsigned long long)run.sorted_pieces, (unsigned long long)runs_chained, (unsigned long long)spills, run.sort_s, run.sgather_s, merge_s);
	if (rc == 0 && sorted && (flags & AL_LIFT_WRITE_INDEX)) {          // the output is closed: the bam-index function over it, with the backend that lifted
		rc = al_bai_index_file(bam_out, nullptr, strcmp(backend, "host twin") == 0, device, n_threads, piece_bytes_arg, nullptr, nullptr, nullptr);
		if (rc) fprintf(stderr, "[airlift] lift: '%s' is written, its index is not\n", bam_out);
	}
	return rc;
}

// ---- test taps (airlift_amd/capi.py) ------------------------------------------------------------------------------------------------------------------------------
// One uncompressed BAM stream (header and records) and a chain file through ONE pass of a backend: the text is the stream as given, the walk starts behind the
// header.  0; -1 a device failure; -3 room (the counts are set); -4 the chain file or the header is refused (its message printed).
static int lift_tap_prepare(const void *bam, size_t n, const char *chain_fn, AlLiftChain &C, AlLiftHeader &H, size_t *start)
{
	std::string err;
	if (al_lift_build(chain_fn, C, err)) { fprintf(stderr, "[ERROR] airlift: %s\n", err.c_str()); return -4; }
	if (al_lift_header_parse((const uint8_t *)bam, n, H, start, err) != 0) { fprintf(stderr, "ERROR: the header is cut or malformed: %s\n", err.c_str()); return -4; }
	if (al_lift_bind(C, H, err)) { fprintf(stderr, "[ERROR] airlift: lift: %s\n", err.c_str()); return -4; }
	return 0;
}
static int lift_tap(AlLiftBackend &B, const void *bam, size_t n, size_t start, uint32_t *rec_off, uint32_t *verdict, size_t rec_cap, uint64_t *out4, void *packed, size_t packed_cap, size_t *packed_n, void *arena, size_t arena_cap, size_t *arena_n)
{
	AlLiftPiece r; const uint8_t *p = nullptr, *a = nullptr;
	if (B.begin(0, n + 1) || B.append(0, (const uint8_t *)bam, n) || B.run(0, start, &r)) return -1;
	out4[0] = r.n_rec; out4[1] = r.consumed; out4[2] = r.first_bad != ~0ull ? r.first_bad : r.walk_bad ? r.n_rec : ~0ull; out4[3] = r.first_bad != ~0ull ? r.bad_code : r.walk_bad ? AL_LIFT_BAD_SIZE : 0;
	*packed_n = (size_t)r.kept_bytes; *arena_n = (size_t)r.arena_bytes;
	if (r.n_rec > rec_cap || r.kept_bytes > packed_cap || r.arena_bytes > arena_cap) return -3;
	if (B.fetch_records(0, rec_off, verdict, (size_t)r.n_rec)) return -1;
	if (r.first_bad != ~0ull) { *packed_n = *arena_n = 0; return 0; }
	if (B.gather(0, r, true) || B.finish(0, &p, &a)) return -1;
	if (r.kept_bytes) memcpy(packed, p, (size_t)r.kept_bytes);
	if (r.arena_bytes) memcpy(arena, a, (size_t)r.arena_bytes);
	return 0;
}
// the sorted form: perm[0, sort3[0]): the record index of every packed record; sort3: packed records, descents, 1 when a sort was launched
static int lift_tap_sorted(AlLiftBackend &B, const void *bam, size_t n, size_t start, uint32_t *rec_off, uint32_t *verdict, size_t rec_cap, uint64_t *out4, void *packed, size_t packed_cap, size_t *packed_n, void *arena, size_t arena_cap, size_t *arena_n,
                           uint32_t *perm, uint64_t *sort3)
{
	AlLiftPiece r; const uint8_t *p = nullptr, *a = nullptr;
	B.set_sorted(true);
	sort3[0] = sort3[1] = sort3[2] = 0;
	if (B.begin(0, n + 1) || B.append(0, (const uint8_t *)bam, n) || B.run(0, start, &r)) return -1;
	out4[0] = r.n_rec; out4[1] = r.consumed; out4[2] = r.first_bad != ~0ull ? r.first_bad : r.walk_bad ? r.n_rec : ~0ull; out4[3] = r.first_bad != ~0ull ? r.bad_code : r.walk_bad ? AL_LIFT_BAD_SIZE : 0;
	*packed_n = (size_t)r.kept_bytes; *arena_n = (size_t)r.arena_bytes;
	if (r.n_rec > rec_cap || r.kept_bytes > packed_cap || r.arena_bytes > arena_cap) return -3;
	if (B.fetch_records(0, rec_off, verdict, (size_t)r.n_rec)) return -1;
	if (r.first_bad != ~0ull) { *packed_n = *arena_n = 0; return 0; }
	if (B.gather(0, r, true) || B.finish(0, &p, &a) || B.fetch_perm(0, perm, (size_t)r.n_packed())) return -1;
	sort3[0] = r.n_packed(); sort3[1] = r.descents; sort3[2] = B.sort_launched(0) ? 1 : 0;
	const uint64_t *keys = nullptr; const uint32_t *lens = nullptr;
	if (B.sorted_out(0, &keys, &lens)) return -1;
	uint64_t sum = 0;
	for (size_t i = 0; i < (size_t)r.n_packed(); ++i) { sum += lens[i]; if (i && keys[i] < keys[i - 1]) { fprintf(stderr, "[airlift] lift --sorted: the keys of the packed records descend at %zu\n", i); return -1; } }
	if (sum != r.kept_bytes) { fprintf(stderr, "[airlift] lift --sorted: the lengths of the packed records sum to %llu, not %llu\n", (unsigned long long)sum, (unsigned long long)r.kept_bytes); return -1; }
	if (r.kept_bytes) memcpy(packed, p, (size_t)r.kept_bytes);
	if (r.arena_bytes) memcpy(arena, a, (size_t)r.arena_bytes);
	return 0;
}
extern "C" int al_dbg_lift_sorted_host(const void *bam, size_t n, const char *chain_fn, uint32_t *rec_off, uint32_t *verdict, size_t rec_cap, uint64_t *out4, void *packed, size_t packed_cap, size_t *packed_n, void *arena, size_t arena_cap, size_t *arena_n,
                                       uint32_t *perm, uint64_t *sort3)
{
	AlLiftChain C; AlLiftHeader H; size_t start = 0;
	if (const int r = lift_tap_prepare(bam, n, chain_fn, C, H, &start)) return r;
	AlLiftHostBackend B(C.tab());
	return lift_tap_sorted(B, bam, n, start, rec_off, verdict, rec_cap, out4, packed, packed_cap, packed_n, arena, arena_cap, arena_n, perm, sort3);
}
// tap_flags & 1: the sort's temporaries count as refused (the order of a piece with a descent is then made on the host, and no sort is launched)
extern "C" int al_dbg_lift_sorted(int device, const void *bam, size_t n, const char *chain_fn, uint32_t *rec_off, uint32_t *verdict, size_t rec_cap, uint64_t *out4, void *packed, size_t packed_cap, size_t *packed_n, void *arena, size_t arena_cap, size_t *arena_n,
                                  uint32_t *perm, uint64_t *sort3, unsigned tap_flags, size_t *held)
{
	AlLiftChain C; AlLiftHeader H; size_t start = 0;
	*held = 0;
	if (const int r = lift_tap_prepare(bam, n, chain_fn, C, H, &start)) return r;
	if (n >= ((size_t)1 << 31) - 65536) return -3;
	std::atomic<size_t> acct{0}; int rc;
	{
		AlLiftDevBackend B; B.acct = &acct; B.refuse_tmp = (tap_flags & 1u) != 0;
		if (B.open(device, C, n / 2 + 1, 0, 0)) return -1;
		rc = lift_tap_sorted(B, bam, n, start, rec_off, verdict, rec_cap, out4, packed, packed_cap, packed_n, arena, arena_cap, arena_n, perm, sort3);
	}
	*held = acct.load();
	return rc;
}
extern "C" int al_dbg_lift_host(const void *bam, size_t n, const char *chain_fn, uint32_t *rec_off, uint32_t *verdict, size_t rec_cap, uint64_t *out4, void *packed, size_t packed_cap, size_t *packed_n, void *arena, size_t arena_cap, size_t *arena_n)
{
	AlLiftChain C; AlLiftHeader H; size_t start = 0;
	if (const int r = lift_tap_prepare(bam, n, chain_fn, C, H, &start)) return r;
	AlLiftHostBackend B(C.tab());
	return lift_tap(B, bam, n, start, rec_off, verdict, rec_cap, out4, packed, packed_cap, packed_n, arena, arena_cap, arena_n);
}
extern "C" int al_dbg_lift(int device, const void *bam, size_t n, const char *chain_fn, uint32_t *rec_off, uint32_t *verdict, size_t rec_cap, uint64_t *out4, void *packed, size_t packed_cap, size_t *packed_n, void *arena, size_t arena_cap, size_t *arena_n, size_t *held)
{
	AlLiftChain C; AlLiftHeader H; size_t start = 0;
	*held = 0;
	if (const int r = lift_tap_prepare(bam, n, chain_fn, C, H, &start)) return r;
	if (n >= ((size_t)1 << 31) - 65536) return -3;
	std::atomic<size_t> acct{0}; int rc;
	{
		AlLiftDevBackend B; B.acct = &acct;
		if (B.open(device, C, n / 2 + 1, 0, 0)) return -1;
		rc = lift_tap(B, bam, n, start, rec_off, verdict, rec_cap, out4, packed, packed_cap, packed_n, arena, arena_cap, arena_n);
	}
	*held = acct.load();
	return rc;
}

// al_chainexact.hip -- chain-exact verify|build: run/1_build_exact_chain_file.py on the GPU (the function: al_dev_chainexact.h).
//
//   k_cex_fold      A-Z of both texts lowered in place, 16 bytes per lane: the compare of '+' blocks is then an XOR of 16-byte words
//   (scan)          segmented sums of (size + dt, size + dq) over the blocks of every chain (al_cex_sum_op): each block's first base in both texts
//   (scan)          exclusive sum of ceil(size / AL_CEX_TILE): the tile table; a tile finds its block by binary search
//   k_cex_count     wavefront per tile: the old side in aligned 16-byte words, the new side assembled from two aligned words (its residue mod 16 is
//                   independent); a 16-bit mismatch mask per word, popcount, wavefront sum: per-tile count, per-block count (one atomic per tile), error flag
//   (scan)          exclusive sums of the tile counts and of the block counts
//   k_cex_emit      the same pass again ('build' only): the positions {block, idx} in order at the scanned offsets
//   k_cex_lines     lane per pass-1 line: mismatch m of block b is line m + b, the block's closing line is at (first mismatch of block b + 1) + b
//   (scan)          pass 2: segmented sums keyed by the last kept line (al_cex_p2_elem), exclusive sum of the head flags
//   k_cex_compact   one line per segment: the head writes size / three / chain, the segment's last element the two sums
// A word of a text is loaded whole only when it lies whole inside the text; the text's last partial word is read byte by byte.  Only the counts, the flag and
// the folded lines are copied to the host (the test taps also take the positions and the pass-1 lines).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <fcntl.h>
#include <unistd.h>
#include <chrono>
#include "al_internal.h"
#include "al_device.h"
#include "al_runtime.h"
#include "al_dev_chainexact.h"
#include "al_prim.h"
#include "../../include/airlift.h"

// A-Z of the four bytes of v lowered: a byte is upper case when its low seven bits are in ['A', 'Z'] and its top bit is clear
__device__ __forceinline__ uint32_t cex_fold4(uint32_t v)
{
	const uint32_t h = v & 0x7f7f7f7fu;
	const uint32_t up = (h + 0x3f3f3f3fu) & ~(h + 0x25252525u) & ~v & 0x80808080u;
	return v | (up >> 2);
}
__global__ void __launch_bounds__(256)
k_cex_fold(uint8_t *__restrict__ t, uint64_t n)
{
	const uint64_t nw = n >> 4, stride = (uint64_t)gridDim.x * blockDim.x, g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	uint4 *w = (uint4 *)t;
	for (uint64_t i = g; i < nw; i += stride) {
		uint4 v = w[i];
		v.x = cex_fold4(v.x); v.y = cex_fold4(v.y); v.z = cex_fold4(v.z); v.w = cex_fold4(v.w);
		w[i] = v;
	}
	if (g < (n & 15)) t[(nw << 4) + g] = al_cex_lower(t[(nw << 4) + g]);
}

// word w (16 bytes) of a text of n bytes: zero outside, byte by byte where the word is the text's last, partial one
__device__ __forceinline__ uint4 cex_ld16(const uint8_t *__restrict__ t, uint64_t n, int64_t w)
{
	uint4 v = make_uint4(0, 0, 0, 0);
	if (w < 0) return v;
	const uint64_t o = (uint64_t)w << 4;
	if (o + 16 <= n) return *(const uint4 *)(t + o);
	if (o < n) {
		uint32_t d[4] = {0, 0, 0, 0};
		for (uint32_t j = 0; j < 16; ++j) if (o + j < n) d[j >> 2] |= (uint32_t)t[o + j] << (8 * (j & 3));
		v = make_uint4(d[0], d[1], d[2], d[3]);
	}
	return v;
}
// bytes [r, r + 16) of the 32 bytes lo:hi
__device__ __forceinline__ uint4 cex_funnel(const uint4 &lo, const uint4 &hi, uint32_t r)
{
	const uint32_t D[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
	const uint32_t q = r >> 2, s = (r & 3) * 8;
	uint32_t E[5], o[4];
#pragma unroll
	for (int k = 0; k < 5; ++k) E[k] = q == 0 ? D[k] : q == 1 ? D[k + 1] : q == 2 ? D[k + 2] : D[k + 3];
#pragma unroll
	for (int k = 0; k < 4; ++k) o[k] = (uint32_t)(((((uint64_t)E[k + 1]) << 32) | E[k]) >> s);
	return make_uint4(o[0], o[1], o[2], o[3]);
}
// bit j: byte j of x is not zero
__device__ __forceinline__ uint32_t cex_nz4(uint32_t x)
{
	const uint32_t hi = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
	return (((hi >> 7) * 0x00204081u) >> 21) & 0xfu;
}
__device__ __forceinline__ uint32_t cex_byte(const uint4 &v, uint32_t j)
{
	const uint32_t d = j < 4 ? v.x : j < 8 ? v.y : j < 12 ? v.z : v.w;
	return (d >> (8 * (j & 3))) & 0xffu;
}
__device__ __forceinline__ uint4 cex_shfl_down1(const uint4 &v)
{
	return make_uint4(__shfl_down(v.x, 1), __shfl_down(v.y, 1), __shfl_down(v.z, 1), __shfl_down(v.w, 1));
}

struct CexArgs {
	const uint8_t *old_text, *new_text; uint64_t n_old, n_new;
	const AlCexLine *line; const AlCexSum *sums; const AlCexChain *chain; uint32_t n_blk, n_chain;
	const uint32_t *tile_first; uint32_t n_tiles;
};

// one tile by one wavefront.  EMIT: the positions at pos[tile_off[t] ...]; otherwise the counts
template <bool EMIT> __device__ __forceinline__ void cex_tile(const CexArgs &A, uint32_t t, uint32_t lane, uint32_t *__restrict__ tile_cnt, uint32_t *__restrict__ blk_cnt, uint32_t *__restrict__ flag,
                                                              const uint32_t *__restrict__ tile_off, AlCexPos *__restrict__ pos, uint32_t n_pos)
{
	uint32_t lo = 0, hi = A.n_blk;                                       // the last block b with tile_first[b] <= t (tile_first[n_blk] = n_tiles > t)
	while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (A.tile_first[mid] <= t) lo = mid; else hi = mid; }
	const uint32_t b = lo;
	const AlCexLine l = A.line[b];
	if (l.chain >= A.n_chain) { if (lane == 0) atomicOr(flag, 2u); return; }   // never happens (the host made the table); never silent, never out of bounds
	const AlCexChain c = A.chain[l.chain];
	uint64_t old_off, new_off; al_cex_off(l, c, A.sums[b], &old_off, &new_off);
	const uint32_t i0 = (t - A.tile_first[b]) * AL_CEX_TILE;
	if (i0 >= l.size) { if (lane == 0) atomicOr(flag, 2u); return; }
	const uint32_t len = l.size - i0 < AL_CEX_TILE ? l.size - i0 : AL_CEX_TILE;
	const uint64_t a0 = old_off + i0;
	const bool minus = c.dir != 0;
	// the whole tile inside both texts, or nothing is read
	bool ok = a0 + len <= A.n_old;
	if (!minus) ok = ok && new_off + i0 + len <= A.n_new; else ok = ok && new_off < A.n_new && new_off + 1 >= (uint64_t)i0 + len;
	if (!ok) { if (lane == 0) atomicOr(flag, 2u); return; }
	const int64_t b0 = minus ? (int64_t)(new_off - i0) : (int64_t)(new_off + i0);   // the new-side position of the tile's first base
	const uint64_t w0 = a0 >> 4, w1 = (a0 + len - 1) >> 4;
	uint32_t total = 0, bad = 0;
	for (uint64_t wb = w0; wb <= w1; wb += 64) {
		const uint64_t w = wb + lane;
		const bool in = w <= w1;
		const uint64_t ws = w << 4;
		const uint32_t vlo = a0 > ws ? (uint32_t)(a0 - ws) : 0u, vhi = a0 + len < ws + 16 ? (uint32_t)(a0 + len - ws) : 16u;   // the word's bytes [vlo, vhi) are of the tile
		const uint32_t valid = in ? ((1u << vhi) - 1u) & ~((1u << vlo) - 1u) : 0u;
		const uint4 o = in ? cex_ld16(A.old_text, A.n_old, (int64_t)w) : make_uint4(0, 0, 0, 0);
		uint32_t m16 = 0;
		if (!minus) {
			const int64_t p = (int64_t)ws + (b0 - (int64_t)a0);              // the new-side position of the word's byte 0
			const int64_t q = p >> 4; const uint32_t r = (uint32_t)(p & 15);
			const uint4 n0 = cex_ld16(A.new_text, A.n_new, q);               // (every lane: lane + 1's word is this lane's upper half)
			uint4 n1 = cex_shfl_down1(n0);
			if (lane == 63) n1 = cex_ld16(A.new_text, A.n_new, q + 1);
			const uint4 nw = cex_funnel(n0, n1, r);
			m16 = cex_nz4(o.x ^ nw.x) | cex_nz4(o.y ^ nw.y) << 4 | cex_nz4(o.z ^ nw.z) << 8 | cex_nz4(o.w ^ nw.w) << 12;
		} else {
			const int64_t p = b0 - ((int64_t)ws - (int64_t)a0) - 15;         // the new side of the word's bytes 15 .. 0 lies at p .. p + 15
			const int64_t q = p >> 4; const uint32_t r = (uint32_t)(p & 15);
			const uint4 nw = cex_funnel(cex_ld16(A.new_text, A.n_new, q), cex_ld16(A.new_text, A.n_new, q + 1), r);
#pragma unroll
			for (uint32_t j = 0; j < 16; ++j) {
				const uint32_t cb = al_cex_comp((uint8_t)cex_byte(nw, 15 - j));
				if ((valid >> j & 1) && cb == 0xff) bad = 1;
				m16 |= (cb != cex_byte(o, j) ? 1u : 0u) << j;
			}
		}
		m16 &= valid;
		const uint32_t k = __popc(m16);
		uint32_t inc = k;                                                    // inclusive sum over the wavefront
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(inc, d); if (lane >= (uint32_t)d) inc += v; }
		if (EMIT) {
			uint32_t at = tile_off[t] + total + inc - k;
			const uint32_t idx0 = i0 + (uint32_t)((int64_t)ws - (int64_t)a0);   // idx of the word's byte 0 (wraps below 0 only for bytes that are not valid)
			for (uint32_t m = m16; m; m &= m - 1) { if (at < n_pos) pos[at] = AlCexPos{b, idx0 + (uint32_t)__builtin_ctz(m)}; ++at; }
		}
		total += __shfl(inc, 63);
	}
	if (!EMIT) {
#pragma unroll
		for (int d = 32; d; d >>= 1) bad |= __shfl_xor(bad, d);
		if (lane == 0) {
			tile_cnt[t] = total;
			if (total) atomicAdd(blk_cnt + b, total);
			if (bad) atomicOr(flag, 1u);
		}
	}
}
__global__ void __launch_bounds__(256)
k_cex_count(const CexArgs A, uint32_t *__restrict__ tile_cnt, uint32_t *__restrict__ blk_cnt, uint32_t *__restrict__ flag)
{
	const uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (t >= A.n_tiles) return;
	cex_tile<false>(A, t, threadIdx.x & 63, tile_cnt, blk_cnt, flag, nullptr, nullptr, 0);
}
__global__ void __launch_bounds__(256)
k_cex_emit(const CexArgs A, const uint32_t *__restrict__ tile_off, AlCexPos *__restrict__ pos, uint32_t n_pos, uint32_t *__restrict__ flag)
{
	const uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (t >= A.n_tiles) return;
	cex_tile<true>(A, t, threadIdx.x & 63, nullptr, nullptr, flag, tile_off, pos, n_pos);
}
__global__ void __launch_bounds__(256)
k_cex_lines(const AlCexLine *__restrict__ line, uint32_t n_blk, const AlCexPos *__restrict__ pos, uint32_t n_pos, const uint32_t *__restrict__ blk_first /* [n_blk + 1] */, AlCexLine *__restrict__ out, uint32_t n_out,
            uint32_t *__restrict__ flag)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_pos + n_blk) return;
	if (i < n_pos) {
		const uint32_t b = pos[i].block;
		if (b >= n_blk || i + b >= n_out || blk_first[b] > i) { atomicOr(flag, 2u); return; }
		out[i + b] = al_cex_line_mis(line[b], pos, i, blk_first[b]);
	} else {
		const uint32_t b = i - n_pos, at = blk_first[b + 1] + b;
		if (at >= n_out || blk_first[b + 1] > n_pos || blk_first[b] > blk_first[b + 1]) { atomicOr(flag, 2u); return; }
		out[at] = al_cex_line_close(line[b], pos, blk_first[b], blk_first[b + 1]);
	}
}
__global__ void __launch_bounds__(256)
k_cex_compact(const AlCexLine *__restrict__ l, const AlCexSum *__restrict__ s, const uint32_t *__restrict__ idx /* [n + 1] */, uint32_t n, uint32_t M, AlCexLine *__restrict__ out)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint32_t k = idx[i], k_next = idx[i + 1];
	const bool head = k_next != k, last = i + 1 == n || idx[i + 2] != k_next;
	const uint32_t r = head ? k : k - 1;                                  // (element 0 is a head, so k >= 1 where i is none; r < idx[n] <= n)
	if (head) { const AlCexLine h = al_cex_p2_out(l[i], M); out[r].chain = h.chain; out[r].size = h.size; out[r].three = h.three; }
	if (last) { out[r].dt = (uint32_t)(s[i].a & ~AL_CEX_F); out[r].dq = (uint32_t)s[i].b; }
}

struct CexSumOp { __host__ __device__ AlCexSum operator()(const AlCexSum &a, const AlCexSum &b) const { return al_cex_sum_op(a, b); } };
struct CexOffIn { const AlCexLine *l; __host__ __device__ AlCexSum operator()(uint32_t i) const { return al_cex_off_elem(l, i); } };
struct CexTilesIn { const AlCexLine *l; uint32_t n; __host__ __device__ uint32_t operator()(uint32_t i) const { return i < n ? (l[i].size + AL_CEX_TILE - 1) / AL_CEX_TILE : 0u; } };
struct CexCntIn { const uint32_t *c; uint32_t n; __host__ __device__ uint32_t operator()(uint32_t i) const { return i < n ? c[i] : 0u; } };
struct CexP2In { const AlCexLine *l; uint32_t M; __host__ __device__ AlCexSum operator()(uint32_t i) const { return al_cex_p2_elem(l, i, M); } };
struct CexHeadIn { const AlCexLine *l; uint32_t n, M; __host__ __device__ uint32_t operator()(uint32_t i) const { return i < n && al_cex_p2_head(l, i, M) ? 1u : 0u; } };

#define CEX_CHECK(x) AL_HIP_CHECK_AS("chainexact", x)
#define CEX_LAUNCH(kern, n, ...) kern<<<dim3(((uint32_t)(n) + 255) / 256), dim3(256), 0, s>>>(__VA_ARGS__)

namespace {
struct ChainExactDev {
	uint8_t *d_old = nullptr, *d_new = nullptr;                            // exactly the texts' sizes: al_dev_malloc, not a DevBuf with its headroom
	DevBuf<AlCexLine> line, l1, l2; DevBuf<AlCexChain> chain; DevBuf<AlCexSum> sums, sums2; DevBuf<uint32_t> tile_first, tile_cnt, tile_off, blk_cnt, blk_first, idx, flag;
	DevBuf<AlCexPos> pos; DevBuf<uint8_t> tmp;
	hipEvent_t ev[7] = {}; hipStream_t s = 0;          // start, texts folded, around k_cex_count, around k_cex_emit, end
	~ChainExactDev()
	{
		(void)hipDeviceSynchronize();
		if (d_old) al_dev_free(d_old);
		if (d_new) al_dev_free(d_new);
		line.release(); l1.release(); l2.release(); chain.release(); sums.release(); sums2.release(); tile_first.release(); tile_cnt.release(); tile_off.release(); blk_cnt.release(); blk_first.release();
		idx.release(); flag.release(); pos.release(); tmp.release();
		for (hipEvent_t &e : ev) if (e) (void)hipEventDestroy(e);
	}
	template <class In> int excl(In in, uint32_t *out, uint32_t n_plus_1)
	{
		auto it = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint32_t>(0u), in);
		return al_prim_run(tmp, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, it, out, 0u, (size_t)n_plus_1, rocprim::plus<uint32_t>(), s); }, "chainexact");
	}
	template <class In> int seg(In in, AlCexSum *out, uint32_t n)
	{
		auto it = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint32_t>(0u), in);
		return al_prim_run(tmp, [&](void *t, size_t &b) { return rocprim::inclusive_scan(t, b, it, out, (size_t)n, CexSumOp(), s); }, "chainexact");
	}
	int text_up(uint8_t **d, const uint8_t *h, uint64_t n)
	{
		if (al_dev_malloc((void **)d, n ? n : 1) != hipSuccess) { (void)hipGetLastError(); *d = nullptr; fprintf(stderr, "[airlift] chainexact: device allocation of %llu bytes failed\n", (unsigned long long)n); return AL_ERR_NOMEM; }
		if ((uintptr_t)*d & 15) { fprintf(stderr, "[airlift] chainexact: a device range is not 16-byte aligned\n"); return -1; }
		if (n) CEX_CHECK(hipMemcpy(*d, h, n, hipMemcpyHostToDevice));
		return 0;
	}
	int run(const AlCexIn &in, bool build, uint32_t M, bool taps, AlCexOut &o);
};

int ChainExactDev::run(const AlCexIn &in, bool build, uint32_t M, bool taps, AlCexOut &o)
{
	const char *why = al_cex_in_bad(in, build);
	if (why) { fprintf(stderr, "[airlift] chainexact: %s\n", why); return -1; }
	const uint32_t n = (uint32_t)in.n;
	o.cnt.assign(n, 0); o.pos.clear(); o.lines1.clear(); o.lines2.clear(); o.flag = 0;
	if (n == 0) return 0;
	for (hipEvent_t &e : ev) CEX_CHECK(hipEventCreate(&e));
	int r;
	const auto t0 = std::chrono::steady_clock::now();
	if ((r = text_up(&d_old, in.old_text, in.n_old)) || (r = text_up(&d_new, in.new_text, in.n_new))) return r;
	if (line.ensure(n) || chain.ensure(in.n_chain) || sums.ensure(n) || tile_first.ensure((size_t)n + 1) || blk_cnt.ensure((size_t)n + 1) || flag.ensure(4)) return AL_ERR_NOMEM;
	CEX_CHECK(hipMemcpy(line.p, in.line, (size_t)n * sizeof(AlCexLine), hipMemcpyHostToDevice));
	CEX_CHECK(hipMemcpy(chain.p, in.chain, (size_t)in.n_chain * sizeof(AlCexChain), hipMemcpyHostToDevice));
	CEX_CHECK(hipMemset(flag.p, 0, 16));
	CEX_CHECK(hipMemset(blk_cnt.p, 0, ((size_t)n + 1) * 4));
	CEX_CHECK(hipDeviceSynchronize());
	o.ms_h2d = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	o.bytes_h2d = in.n_old + in.n_new + (uint64_t)n * sizeof(AlCexLine) + (uint64_t)in.n_chain * sizeof(AlCexChain);
	CEX_CHECK(hipEventRecord(ev[0], s));
	k_cex_fold<<<dim3((uint32_t)std::min<uint64_t>((in.n_old >> 12) + 1, 8192)), dim3(256), 0, s>>>(d_old, in.n_old);
	CEX_CHECK(hipGetLastError());
	k_cex_fold<<<dim3((uint32_t)std::min<uint64_t>((in.n_new >> 12) + 1, 8192)), dim3(256), 0, s>>>(d_new, in.n_new);
	CEX_CHECK(hipGetLastError());
	CEX_CHECK(hipEventRecord(ev[1], s));
	if ((r = seg(CexOffIn{line.p}, sums.p, n)) || (r = excl(CexTilesIn{line.p, n}, tile_first.p, n + 1))) return r;
	uint32_t n_tiles = 0;
	CEX_CHECK(hipMemcpyAsync(&n_tiles, tile_first.p + n, 4, hipMemcpyDeviceToHost, s));
	CEX_CHECK(hipStreamSynchronize(s));
	if (n_tiles == 0 || n_tiles >= AL_CEX_MOST) { fprintf(stderr, "[airlift] chainexact: %u blocks left %u tiles\n", n, n_tiles); return -1; }
	if (tile_cnt.ensure((size_t)n_tiles + 1) || tile_off.ensure((size_t)n_tiles + 1) || blk_first.ensure((size_t)n + 1)) return AL_ERR_NOMEM;
	CexArgs A{d_old, d_new, in.n_old, in.n_new, line.p, sums.p, chain.p, n, in.n_chain, tile_first.p, n_tiles};
	CEX_CHECK(hipEventRecord(ev[2], s));
	k_cex_count<<<dim3((n_tiles + 3) / 4), dim3(256), 0, s>>>(A, tile_cnt.p, blk_cnt.p, flag.p);
	CEX_CHECK(hipGetLastError());
	CEX_CHECK(hipEventRecord(ev[3], s));
	CEX_CHECK(hipMemcpyAsync(o.cnt.data(), blk_cnt.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
	CEX_CHECK(hipMemcpyAsync(&o.flag, flag.p, 4, hipMemcpyDeviceToHost, s));
	CEX_CHECK(hipStreamSynchronize(s));
	o.bytes_d2h = (uint64_t)n * 4 + 8;
	bool emitted = false;
	auto done = [&]() -> int {
		CEX_CHECK(hipEventRecord(ev[6], s));
		CEX_CHECK(hipEventSynchronize(ev[6]));
		float ms = 0; CEX_CHECK(hipEventElapsedTime(&ms, ev[0], ev[6]));
		o.ms_kernels = ms;
		CEX_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1])); o.ms_fold = ms;
		CEX_CHECK(hipEventElapsedTime(&ms, ev[2], ev[3])); o.ms_count = ms;
		if (emitted) { CEX_CHECK(hipEventElapsedTime(&ms, ev[4], ev[5])); o.ms_emit = ms; }
		if (o.flag & 2u) { fprintf(stderr, "[airlift] chainexact: a block, tile or line lies outside its tables\n"); return -1; }
		return 0;
	};
	if (!build || o.flag) return done();
	uint64_t n_mis = 0;
	for (uint32_t i = 0; i < n; ++i) n_mis += o.cnt[i];
	if (n_mis + n >= AL_CEX_MOST) { fprintf(stderr, "[airlift] chainexact: %llu mismatches are more than one run takes\n", (unsigned long long)n_mis); return -1; }
	const uint32_t n_pos = (uint32_t)n_mis, n1 = n_pos + n;
	if (pos.ensure((size_t)n_pos + 1) || l1.ensure(n1) || l2.ensure(n1) || sums2.ensure(n1) || idx.ensure((size_t)n1 + 2)) return AL_ERR_NOMEM;
	if ((r = excl(CexCntIn{tile_cnt.p, n_tiles}, tile_off.p, n_tiles + 1)) || (r = excl(CexCntIn{blk_cnt.p, n}, blk_first.p, n + 1))) return r;
	CEX_CHECK(hipEventRecord(ev[4], s));
	if (n_pos) {
		k_cex_emit<<<dim3((n_tiles + 3) / 4), dim3(256), 0, s>>>(A, (const uint32_t *)tile_off.p, pos.p, n_pos, flag.p);
		CEX_CHECK(hipGetLastError());
	}
	CEX_CHECK(hipEventRecord(ev[5], s));
	emitted = true;
	CEX_LAUNCH(k_cex_lines, n1, (const AlCexLine *)line.p, n, (const AlCexPos *)pos.p, n_pos, (const uint32_t *)blk_first.p, l1.p, n1, flag.p);
	CEX_CHECK(hipGetLastError());
	if ((r = seg(CexP2In{l1.p, M}, sums2.p, n1)) || (r = excl(CexHeadIn{l1.p, n1, M}, idx.p, n1 + 1))) return r;
	CEX_LAUNCH(k_cex_compact, n1, (const AlCexLine *)l1.p, (const AlCexSum *)sums2.p, (const uint32_t *)idx.p, n1, M, l2.p);
	CEX_CHECK(hipGetLastError());
	uint32_t n2 = 0;
	CEX_CHECK(hipMemcpyAsync(&n2, idx.p + n1, 4, hipMemcpyDeviceToHost, s));
	CEX_CHECK(hipMemcpyAsync(&o.flag, flag.p, 4, hipMemcpyDeviceToHost, s));
	CEX_CHECK(hipStreamSynchronize(s));
	if (n2 == 0 || n2 > n1) { fprintf(stderr, "[airlift] chainexact: pass 2 made %u lines of %u\n", n2, n1); return -1; }
	o.lines2.resize(n2);
	CEX_CHECK(hipMemcpy(o.lines2.data(), l2.p, (size_t)n2 * sizeof(AlCexLine), hipMemcpyDeviceToHost));
	o.bytes_d2h += (uint64_t)n2 * sizeof(AlCexLine) + 8;
	if (taps) {
		o.pos.resize(n_pos); o.lines1.resize(n1);
		if (n_pos) CEX_CHECK(hipMemcpy(o.pos.data(), pos.p, (size_t)n_pos * sizeof(AlCexPos), hipMemcpyDeviceToHost));
		CEX_CHECK(hipMemcpy(o.lines1.data(), l1.p, (size_t)n1 * sizeof(AlCexLine), hipMemcpyDeviceToHost));
	}
	return done();
}
}  // namespace

int al_chainexact_device(int device, const AlCexIn &in, bool build, uint32_t M, bool taps, AlCexOut &o)
{
	if (hipSetDevice(device < 0 ? 0 : device) != hipSuccess) { (void)hipGetLastError(); fprintf(stderr, "[airlift] chainexact: no HIP device %d\n", device < 0 ? 0 : device); return -2; }
	ChainExactDev D;
	const int rc = D.run(in, build, M, taps, o);
	if (rc == 0 && al_env().test_guard && al_dev_guard_check()) fprintf(stderr, "[airlift] GUARD: violations after chainexact\n");
	return rc;
}

// ---- chain-exact -------------------------------------------------------------------------------------------------------------------------------------------------
// the line of the file's first 'U' or 'u' outside a header line (the loader would make it a 't', and the script compares it as written): 0 for none, -1: unreadable
static long long cex_first_u(const char *fn)
{
	const int fd = open(fn, O_RDONLY);
	if (fd < 0) return -1;
	struct stat st;
	if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) { close(fd); return -1; }
	if (st.st_size == 0) { close(fd); return 0; }
	const char *d = (const char *)mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
	close(fd);
	if (d == MAP_FAILED) return -1;
	long long line = 0, found = 0;
	for (const char *p = d, *e = d + st.st_size; p < e && !found;) {
		const char *nl = (const char *)memchr(p, '\n', (size_t)(e - p)), *q = nl ? nl : e;
		++line;
		if (*p != '>' && (memchr(p, 'U', (size_t)(q - p)) || memchr(p, 'u', (size_t)(q - p)))) found = line;
		p = q + 1;
	}
	munmap((void *)d, (size_t)st.st_size);
	return found;
}
static int cex_load(const char *fn, std::vector<AlSeq> &seqs, AlText &text, AlCexFa &fa)
{
	const long long u = cex_first_u(fn);
	if (u < 0) { fprintf(stderr, "[ERROR] airlift: %s: cannot be opened\n", fn); return -1; }
	if (u > 0) { fprintf(stderr, "[ERROR] airlift: %s:%lld: a 'U' or 'u' among the bases\n", fn, u); return -1; }
	if (!al_fasta_load_parallel(fn, 8, seqs, text)) { fprintf(stderr, "[ERROR] airlift: %s: not a plain FASTA file\n", fn); return -1; }
	for (const AlSeq &q : seqs) { fa.name.push_back(q.name); fa.off.push_back(q.offset); fa.len.push_back(q.len); }
	fa.text = (const uint8_t *)text.data(); fa.n = text.size();
	const std::string *twice = fa.index();
	if (twice) { fprintf(stderr, "[ERROR] airlift: %s: the contig '%s' appears twice\n", fn, twice->c_str()); return -1; }
	return 0;
}

extern "C" int al_chain_exact(const char *old_fa, const char *new_fa, const char *chain_fn, int mode, int min_region, FILE *out, unsigned flags, int device)
{
	if (!old_fa || !new_fa || !chain_fn || !out) { fprintf(stderr, "[ERROR] airlift: al_chain_exact needs two FASTA files, a chain file and an output\n"); return -1; }
	if (mode != AL_CEX_VERIFY && mode != AL_CEX_BUILD) { fprintf(stderr, "[ERROR] airlift: al_chain_exact: the mode is verify (0) or build (1)\n"); return -1; }
	if (min_region < 1 || min_region > (1 << 30)) { fprintf(stderr, "[ERROR] airlift: al_chain_exact: the smallest region (--min-region) must be positive\n"); return -1; }
	typedef std::chrono::steady_clock clk;
	auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
	AlCexTab tab; std::string err;
	if (al_cex_parse(chain_fn, tab, err) != 0) { fprintf(stderr, "[ERROR] airlift: %s\n", err.c_str()); return -1; }
	const auto t_load = clk::now();
	std::vector<AlSeq> so, sn; AlText to, tn; AlCexFa fo, fn;
	if (cex_load(old_fa, so, to, fo) != 0 || cex_load(new_fa, sn, tn, fn) != 0) return -1;
	const double ms_load = ms_since(t_load);
	AlCexRun run;
	if (al_cex_table(chain_fn, tab, fo, fn, mode, run, err) != 0) { fprintf(stderr, "[ERROR] airlift: %s\n", err.c_str()); return -1; }
	AlCexIn in; in.old_text = fo.text; in.n_old = fo.n; in.new_text = fn.text; in.n_new = fn.n; in.n = run.line.size(); in.line = run.line.data(); in.n_chain = (uint32_t)run.chain.size(); in.chain = run.chain.data();
	const bool build = mode == AL_CEX_BUILD;
	const char *why = al_cex_in_bad(in, build);
	if (why) { fprintf(stderr, "[ERROR] airlift: %s: %s\n", chain_fn, why); return -1; }
	AlCexOut o;
	const auto t_run = clk::now();
	if (flags & AL_CHAIN_HOST) al_chainexact_host(in, build, (uint32_t)min_region, o);
	else { const int rc = al_chainexact_device(device, in, build, (uint32_t)min_region, false, o); if (rc != 0) return rc; }
	const double ms_run = ms_since(t_run);
	if (o.flag) {
		const unsigned long long ln = al_cex_flag_line(in, run);
		fprintf(stderr, "[ERROR] airlift: %s:%llu: a block of a '-' chain compares a new-side byte other than acgtnACGTN\n", chain_fn, ln);
		return -1;
	}
	const auto t_text = clk::now();
	std::string text;
	if (build) al_cex_build_text(tab, o.lines2, text); else al_cex_verify_text(tab, run, o.cnt, text);
	const bool bad_write = fwrite(text.data(), 1, text.size(), out) != text.size() || fflush(out) == EOF;
	if (al_env().timing) {
		uint64_t bases = 0, mis = 0;
		for (size_t i = 0; i < run.line.size(); ++i) { bases += run.line[i].size; mis += o.cnt[i]; }
		if (flags & AL_CHAIN_HOST) fprintf(stderr, "[airlift] chainexact: %zu blocks, %llu bases, %llu mismatches, %zu lines; load %.3f ms; host twin %.3f ms; text %.3f ms\n", run.line.size(), (unsigned long long)bases,
		                                   (unsigned long long)mis, o.lines2.size(), ms_load, ms_run, ms_since(t_text));
		else fprintf(stderr, "[airlift] chainexact: %zu blocks, %llu bases, %llu mismatches, %zu lines; load %.3f ms; to the device %.3f ms (%llu bytes); kernels %.3f ms (fold %.3f, count %.3f, emit %.3f); device pass %.3f ms; from the device %llu bytes; text %.3f ms\n",
		             run.line.size(), (unsigned long long)bases, (unsigned long long)mis, o.lines2.size(), ms_load, o.ms_h2d, (unsigned long long)o.bytes_h2d, o.ms_kernels, o.ms_fold, o.ms_count, o.ms_emit, ms_run, (unsigned long long)o.bytes_d2h, ms_since(t_text));
	}
	return bad_write ? -3 : 0;
}

// ---- test taps ---------------------------------------------------------------------------------------------------------------------------------------------------
static int cex_tap(bool dev, const uint8_t *old_text, uint64_t n_old, const uint8_t *new_text, uint64_t n_new, uint64_t n, const uint32_t *chain, const uint32_t *size, const uint32_t *dt, const uint32_t *dq,
                   const uint32_t *three, uint32_t n_chain, const uint64_t *c_old0, const uint64_t *c_new0, const uint32_t *c_dir, int build, int min_region, uint32_t *o_cnt, uint32_t *o_pos, uint64_t cap_pos,
                   uint64_t *n_pos, uint32_t *o_l1, uint64_t cap_l1, uint64_t *n_l1, uint32_t *o_l2, uint64_t cap_l2, uint64_t *n_l2, uint32_t *o_flag)
{
	if ((n && (!chain || !size || !dt || !dq || !three || !o_cnt)) || (n_chain && (!c_old0 || !c_new0 || !c_dir)) || !o_flag || min_region < 1 || min_region > (1 << 30)) return -1;
	if (build && (!n_pos || !n_l1 || !n_l2 || (cap_pos && !o_pos) || (cap_l1 && !o_l1) || (cap_l2 && !o_l2))) return -1;
	std::vector<AlCexLine> line(n); std::vector<AlCexChain> ch(n_chain);
	for (uint64_t i = 0; i < n; ++i) line[i] = al_cex_mk(chain[i], size[i], dt[i], dq[i], three[i]);
	for (uint32_t c = 0; c < n_chain; ++c) { ch[c] = AlCexChain{}; ch[c].old0 = c_old0[c]; ch[c].new0 = c_new0[c]; ch[c].dir = c_dir[c]; }
	AlCexIn in; in.old_text = old_text; in.n_old = n_old; in.new_text = new_text; in.n_new = n_new; in.n = n; in.line = line.data(); in.n_chain = n_chain; in.chain = ch.data();
	const char *why = al_cex_in_bad(in, build != 0);
	if (why) { fprintf(stderr, "[airlift] al_dbg_chainexact: %s\n", why); return -1; }
	AlCexOut o;
	if (dev) {
		int d = 0;
		if (hipGetDevice(&d) != hipSuccess) { (void)hipGetLastError(); fprintf(stderr, "[airlift] al_dbg_chainexact: no HIP device\n"); return -2; }
		const int rc = al_chainexact_device(d, in, build != 0, (uint32_t)min_region, true, o);
		if (rc != 0) return rc;
	} else al_chainexact_host(in, build != 0, (uint32_t)min_region, o);
	*o_flag = o.flag;
	for (uint64_t i = 0; i < n; ++i) o_cnt[i] = o.flag ? 0 : o.cnt[i];
	if (!build) return 0;
	*n_pos = *n_l1 = *n_l2 = 0;
	if (o.flag) return 0;                                                 // nothing is said of a refused input
	if (o.pos.size() > cap_pos || o.lines1.size() > cap_l1 || o.lines2.size() > cap_l2) return -4;
	for (size_t i = 0; i < o.pos.size(); ++i) { o_pos[2 * i] = o.pos[i].block; o_pos[2 * i + 1] = o.pos[i].idx; }
	auto put = [](const std::vector<AlCexLine> &v, uint32_t *p, uint64_t *cnt) { for (size_t i = 0; i < v.size(); ++i) { p[5 * i] = v[i].chain; p[5 * i + 1] = v[i].size; p[5 * i + 2] = v[i].dt; p[5 * i + 3] = v[i].dq; p[5 * i + 4] = v[i].three; } *cnt = v.size(); };
	*n_pos = o.pos.size(); put(o.lines1, o_l1, n_l1); put(o.lines2, o_l2, n_l2);
	return 0;
}
extern "C" int al_dbg_chainexact(const uint8_t *old_text, uint64_t n_old, const uint8_t *new_text, uint64_t n_new, uint64_t n, const uint32_t *chain, const uint32_t *size, const uint32_t *dt, const uint32_t *dq,
                                 const uint32_t *three, uint32_t n_chain, const uint64_t *c_old0, const uint64_t *c_new0, const uint32_t *c_dir, int build, int min_region, uint32_t *o_cnt, uint32_t *o_pos,
                                 uint64_t cap_pos, uint64_t *n_pos, uint32_t *o_l1, uint64_t cap_l1, uint64_t *n_l1, uint32_t *o_l2, uint64_t cap_l2, uint64_t *n_l2, uint32_t *o_flag)
{
	return cex_tap(true, old_text, n_old, new_text, n_new, n, chain, size, dt, dq, three, n_chain, c_old0, c_new0, c_dir, build, min_region, o_cnt, o_pos, cap_pos, n_pos, o_l1, cap_l1, n_l1, o_l2, cap_l2, n_l2, o_flag);
}
extern "C" int al_dbg_chainexact_host(const uint8_t *old_text, uint64_t n_old, const uint8_t *new_text, uint64_t n_new, uint64_t n, const uint32_t *chain, const uint32_t *size, const uint32_t *dt, const uint32_t *dq,
                                      const uint32_t *three, uint32_t n_chain, const uint64_t *c_old0, const uint64_t *c_new0, const uint32_t *c_dir, int build, int min_region, uint32_t *o_cnt, uint32_t *o_pos,
                                      uint64_t cap_pos, uint64_t *n_pos, uint32_t *o_l1, uint64_t cap_l1, uint64_t *n_l1, uint32_t *o_l2, uint64_t cap_l2, uint64_t *n_l2, uint32_t *o_flag)
{
	return cex_tap(false, old_text, n_old, new_text, n_new, n, chain, size, dt, dq, three, n_chain, c_old0, c_new0, c_dir, build, min_region, o_cnt, o_pos, cap_pos, n_pos, o_l1, cap_l1, n_l1, o_l2, cap_l2, n_l2, o_flag);
}
extern "C" uint32_t al_dbg_chainexact_tile(void) { return AL_CEX_TILE; }

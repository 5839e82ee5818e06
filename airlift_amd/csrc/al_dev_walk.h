// al_dev_walk.h -- k_bam_walk: the record offsets of an inflated BAM text along the chain of block_size fields (WALK in al_dev_lift.h).  Device code only:
// al_lift.hip and al_merge.hip both include it, and each gets the kernel in its own code object (hence `static`).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "al_dev_lift.h"       // AL_LIFT_MAX_BS

#define AL_LIFT_W 8192u                       // bytes of a window (a power of two, a multiple of 64 x 16)
#define AL_LIFT_V (AL_LIFT_W / 16 / 64)       // 16-byte loads per lane and window

// window w of the text into a lane's registers; lim: the bytes of the text's buffer that may be read.  A window that lies whole below lim -- every window
// of a text whose buffer has the room begin() asks for -- is loaded without a branch per load, so that the loads stay in flight while the lanes go on.
typedef uint32_t al_u32x4 __attribute__((ext_vector_type(4)));
struct AlWalkRegs { al_u32x4 v[AL_LIFT_V]; };
__device__ __forceinline__ void walk_load(AlWalkRegs &R, const uint8_t *__restrict__ t, uint32_t w, uint32_t lim, uint32_t l)
{
	const al_u32x4 zero = {0, 0, 0, 0};
	if ((uint64_t)(w + 1) * AL_LIFT_W <= lim) {
		_Pragma("unroll")
		for (uint32_t j = 0; j < AL_LIFT_V; ++j) R.v[j] = *(const al_u32x4 *)(t + (size_t)w * AL_LIFT_W + (l + 64 * j) * 16); }
	else {
		_Pragma("unroll")
		for (uint32_t j = 0; j < AL_LIFT_V; ++j) { const uint64_t off = (uint64_t)w * AL_LIFT_W + (l + 64 * j) * 16; R.v[j] = off + 16 <= lim ? *(const al_u32x4 *)(t + off) : zero; }
	}
}
// The hop is uniform: every lane reads the same two LDS words (a broadcast), the size field is taken out of them with one funnel shift and made scalar, so
// the loop's compares and branches are scalar; lane i & 63 keeps the offset of record i and the 64 offsets leave with one store.
static __global__ void __launch_bounds__(64)
k_bam_walk(const uint8_t *__restrict__ t, uint32_t n, uint32_t lim, uint32_t start, uint32_t *__restrict__ rec_off, uint32_t *__restrict__ res)
{
	__shared__ al_u32x4 ring4[2 * AL_LIFT_W / 16];
	const uint32_t *ring32 = (const uint32_t *)ring4;
	const uint32_t l = threadIdx.x;
	uint32_t p = start, n_rec = 0, mine = 0, state = p + 4 > n ? 1u : 0u;   // state 1: the walk has ended; 2: at a block_size out of range
	uint32_t k = p / AL_LIFT_W;
	AlWalkRegs R = {};
	if (state == 0) {
		walk_load(R, t, k, lim, l);
		_Pragma("unroll")
		for (uint32_t j = 0; j < AL_LIFT_V; ++j) ring4[(k & 1) * (AL_LIFT_W / 16) + l + 64 * j] = R.v[j];
	}
	__syncthreads();
	while (state == 0) {
		const bool pre = (uint64_t)(k + 1) * AL_LIFT_W < n;
		if (pre) walk_load(R, t, k + 1, lim, l);
		const uint32_t wend = pre ? (k + 1) * AL_LIFT_W : n;
		while (p + 4 <= wend) {
			const uint32_t a = (p & (2 * AL_LIFT_W - 1)) >> 2;
			const uint32_t lo = ring32[a], hi = ring32[(a + 1) & (2 * AL_LIFT_W / 4 - 1)];
			const uint32_t bs = __builtin_amdgcn_readfirstlane(__funnelshift_r(lo, hi, (p & 3) * 8));
			if (bs < 32 || bs > AL_LIFT_MAX_BS) { state = 2; break; }
			if (p + 4 + bs > n) { state = 1; break; }
			if (l == (n_rec & 63)) mine = p;
			++n_rec;
			if ((n_rec & 63) == 0) rec_off[n_rec - 64 + l] = mine;
			p += 4 + bs;
		}
		if (state == 0 && p + 4 > n) state = 1;
		if (state) break;
		const uint32_t k2 = p / AL_LIFT_W;
		__syncthreads();
		if (k2 <= k + 1) ++k;                                              // (p + 4 lies beyond window k and inside the text: window k + 1 exists and is on its way)
		else { k = k2; walk_load(R, t, k, lim, l); }                       // a record that ends beyond the next window: skipped, the window of p loaded afresh
		_Pragma("unroll")
		for (uint32_t j = 0; j < AL_LIFT_V; ++j) ring4[(k & 1) * (AL_LIFT_W / 16) + l + 64 * j] = R.v[j];
		__syncthreads();
	}
	if (l < (n_rec & 63)) rec_off[(n_rec & ~63u) + l] = mine;
	if (l == 0) { res[0] = n_rec; res[1] = p; res[2] = state == 2 ? 1u : 0u; }
}

// al_deflate.hip -- BGZF blocks deflated on the GPU (--gpu-deflate; product code).  The function computed is the one written down at the head of
// al_dev_deflate.h; this file is its parallel evaluation and the device backend that AlBgzf (al_bam.cpp) drives.
//
// k_deflate: one workgroup of 1024 lanes per BGZF block, persistent (the grid is the device's CU count; a workgroup strides over the block list), so the
// per-position match words in HBM (4 bytes x 0xff00 per workgroup) are sized by the grid.  A block's bytes sit in LDS for the whole time; a second 64 KB
// region of LDS is, in turn, the hash table of step 1, the per-position step bytes the parse walks, and the member as it is put together -- 147 KB of the
// CU's 160 KB in all, one workgroup per CU.  The only serial part is the greedy parse (one lane, over step bytes in LDS) and the two Huffman constructions
// (one lane each, at the same time).  k_dfl_offsets / k_dfl_pack then move the members back to back, so that only compressed bytes cross to the host.
// The input is a stream of two segments: host-held flushes come up whole into one staging buffer (al_deflate_dev_run); a --bam batch of the stream driver is
// compressed where it lies, behind the carry of the batch before, which sits in the seam buffer (al_deflate_dev_run_resident) -- the block that straddles the
// two is gathered byte by byte.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <vector>
#include "al_runtime.h"
#include "al_io.h"
#include "al_bam.h"
#include "al_dev_deflate.h"

namespace {

const uint32_t DFL_T = 1024;                              // lanes per workgroup
const uint32_t DFL_INW = AL_DFL_BLOCK / 4 + 4;            // the block's words in LDS, 16 bytes of padding behind them (the word compares read past the end, never count it)
const uint32_t DFL_UW = AL_DFL_SLOT / 4;

struct DflLds {
	uint32_t in[DFL_INW];
	uint32_t u[DFL_UW];                                    // hash table (position + 1) | step bytes | the member's words
	uint32_t sel[2048];                                    // bit i: position i starts a token
	uint32_t lfreq[288], dfreq[32], A[288], Ad[32];
	uint32_t red[DFL_T];
	uint32_t wsum[16];
	uint32_t misc[8];                                      // 1: used literal/length symbols, 2: used distance symbols, 3: bits of the dynamic form
	uint16_t S[288], Sd[32], lcode[288], dcode[32];
	uint8_t llen[288], dlen[32];
};

struct DflSink {
	uint32_t *w;
	__host__ __device__ void orw(uint32_t i, uint32_t v)
	{
#ifdef __HIP_DEVICE_COMPILE__
		if (v) atomicOr(&w[i], v);
#else
		w[i] |= v;
#endif
	}
};

__device__ __forceinline__ uint32_t ld32(const uint32_t *w, uint32_t i)
{   // the four bytes at byte offset i of a word array
	return __builtin_amdgcn_alignbyte(w[(i >> 2) + 1], w[i >> 2], i & 3);
}

// The stream is s0[0, n0) followed by s1[0, n - n0); block b is its bytes [b * 0xff00, ...).  scratch: gridDim.x * 0xff00 words.
// slots: nb * 65536 bytes, block b's member at b * 65536; sizes[b] its length, stored[b] whether it is a stored block.
__global__ __launch_bounds__(1024) void k_deflate(const uint8_t *s0, uint64_t n0, const uint8_t *s1, uint64_t n, int level, uint32_t *scratch, uint32_t *slots, uint32_t *sizes, uint32_t *stored, uint32_t nb)
{
	__shared__ DflLds L;
	const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	uint32_t *mt = scratch + (size_t)blockIdx.x * AL_DFL_BLOCK;
	const uint8_t *inb = (const uint8_t *)L.in;
	uint8_t *ub = (uint8_t *)L.u;
	for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
		const uint64_t off = (uint64_t)b * AL_DFL_BLOCK;
		const uint32_t bn = (uint32_t)(n - off < AL_DFL_BLOCK ? n - off : AL_DFL_BLOCK);
		// ---- the block into LDS, zero-padded
		{
			const uint8_t *p = off + bn <= n0 ? s0 + off : off >= n0 ? s1 + (off - n0) : nullptr;
			const bool al = p && ((uintptr_t)p & 3) == 0;
			for (uint32_t w = tid; w < DFL_INW; w += DFL_T) {
				uint32_t v = 0;
				if (al && 4 * w + 4 <= bn) v = ((const uint32_t *)p)[w];
				else for (uint32_t k = 0; k < 4; ++k) { const uint64_t g = off + 4 * w + k; if (4 * w + k < bn) v |= (uint32_t)(g < n0 ? s0[g] : s1[g - n0]) << (8 * k); }
				L.in[w] = v;
			}
			for (uint32_t w = tid; w < DFL_UW; w += DFL_T) L.u[w] = 0;
			for (uint32_t w = tid; w < 2048; w += DFL_T) L.sel[w] = 0;
			if (tid < 288) { L.lfreq[tid] = 0; L.llen[tid] = 0; }
			if (tid < 32) { L.dfreq[tid] = 0; L.dlen[tid] = 0; }
			if (tid < 8) L.misc[tid] = 0;
		}
		__syncthreads();
		// ---- CRC32: the block right-aligned in 65536 bytes, 64 per lane, the registers joined pairwise
		{
			const uint32_t pad = AL_DFL_SLOT - bn;
			uint32_t r = 0;
			for (uint32_t v = tid * 64; v < tid * 64 + 64; ++v) { if (v < pad) continue; const uint32_t i = v - pad; if (i == 0) r = 0xffffffffu; r = al_dfl_crc_byte(r, inb[i]); }
			L.red[tid] = r;
			uint32_t xp = al_dfl_crc_xpow8(64);
			for (uint32_t s = 1; s < DFL_T; s <<= 1) {
				__syncthreads();
				if ((tid & (2 * s - 1)) == 0) L.red[tid] = al_dfl_crc_mul(L.red[tid], xp) ^ L.red[tid + s];
				xp = al_dfl_crc_mul(xp, xp);
			}
			__syncthreads();
		}
		const uint32_t crc = ~L.red[0];
		bool huff = level != 0;
		uint32_t comp = 0;
		if (huff) {
			// ---- 1. candidates, a chunk at a time: all look up, then all insert by maximum
			const uint32_t nh = bn >= 4 ? bn - 3 : 0;
			for (uint32_t base = 0; base < nh; base += AL_DFL_CHUNK) {
				const uint32_t i = base + tid; const bool act = tid < AL_DFL_CHUNK && i < nh;
				uint32_t h = 0;
				if (act) { h = al_dfl_hash(ld32(L.in, i)); mt[i] = L.u[h]; }
				__syncthreads();
				if (act) atomicMax(&L.u[h], i + 1);
				__syncthreads();
			}
			// ---- 2. lengths; the table's place becomes the step bytes (0: literal, else length - 3)
			// (the candidates are in mt[] already: nothing reads the table any more)
			for (uint32_t i = tid; i < bn; i += DFL_T) {
				const uint32_t c = i < nh ? mt[i] : 0; uint32_t l = 0;
				if (c && i - (c - 1) <= 32768) {
					const uint32_t cap = bn - i < 258 ? bn - i : 258, j = c - 1;
					while (l < cap) { const uint32_t x = ld32(L.in, j + l) ^ ld32(L.in, i + l); if (x) { l += (uint32_t)__builtin_ctz(x) >> 3; break; } l += 4; }
					if (l > cap) l = cap;
				}
				const uint32_t m = l >= 4 ? l << 16 | (i - (c - 1) - 1) : 0;
				mt[i] = m; ub[i] = m ? (uint8_t)(l - 3) : 0;
			}
			__syncthreads();
			// ---- 3. the greedy parse: one lane walks the step bytes and marks the token starts
			if (tid == 0) {
				uint32_t i = 0, cw = 0, cbits = 0;
				while (i < bn) {
					const uint32_t wi = i >> 2, w = L.u[wi];
					while (i < bn && (i >> 2) == wi) {
						if ((i >> 5) != cw) { L.sel[cw] = cbits; cw = i >> 5; cbits = 0; }
						cbits |= 1u << (i & 31);
						const uint32_t s = (w >> (8 * (i & 3))) & 255;
						i += s ? s + 3 : 1;
					}
				}
				L.sel[cw] = cbits;
			}
			__syncthreads();
			// ---- 4. histograms, code lengths, codes
			for (uint32_t i = tid; i < bn; i += DFL_T) if (L.sel[i >> 5] >> (i & 31) & 1) {
				const uint32_t m = mt[i];
				if (!m) atomicAdd(&L.lfreq[inb[i]], 1u);
				else { uint32_t s, e, v; al_dfl_len_sym(m >> 16, &s, &e, &v); atomicAdd(&L.lfreq[s], 1u); al_dfl_dist_sym((m & 0xffff) + 1, &s, &e, &v); atomicAdd(&L.dfreq[s], 1u); }
			}
			if (tid == 0) atomicAdd(&L.lfreq[256], 1u);
			__syncthreads();
			if (tid < AL_DFL_NLIT) {       // the used symbols in (frequency, symbol) order: each finds its own rank
				const uint32_t f = L.lfreq[tid];
				if (f) { uint32_t r = 0; for (uint32_t t = 0; t < AL_DFL_NLIT; ++t) { const uint32_t g = L.lfreq[t]; r += g && (g < f || (g == f && t < tid)); } L.A[r] = f; L.S[r] = (uint16_t)tid; atomicAdd(&L.misc[1], 1u); }
			} else if (tid >= 512 && tid < 512 + AL_DFL_NDIST) {
				const uint32_t me = tid - 512, f = L.dfreq[me];
				if (f) { uint32_t r = 0; for (uint32_t t = 0; t < AL_DFL_NDIST; ++t) { const uint32_t g = L.dfreq[t]; r += g && (g < f || (g == f && t < me)); } L.Ad[r] = f; L.Sd[r] = (uint16_t)me; atomicAdd(&L.misc[2], 1u); }
			}
			__syncthreads();
			if (tid == 0) { al_dfl_lengths_sorted(L.A, L.S, (int)L.misc[1], L.llen); al_dfl_codes(L.llen, AL_DFL_NLIT, L.lcode); }
			else if (tid == 512) { al_dfl_lengths_sorted(L.Ad, L.Sd, (int)L.misc[2], L.dlen); al_dfl_fix_dist(L.dlen); al_dfl_codes(L.dlen, AL_DFL_NDIST, L.dcode); }
			__syncthreads();
			if (tid < AL_DFL_NLIT) atomicAdd(&L.misc[3], L.lfreq[tid] * (L.llen[tid] + (tid > 256 ? al_dfl_len_extra(tid) : 0)));
			else if (tid >= 512 && tid < 512 + AL_DFL_NDIST) atomicAdd(&L.misc[3], L.dfreq[tid - 512] * (L.dlen[tid - 512] + al_dfl_dist_extra(tid - 512)));
			__syncthreads();
			comp = (AL_DFL_HDRBITS + L.misc[3] + 7) >> 3;
			if (comp >= bn + 5) huff = false;
		}
		// ---- 5. / 6. the member, put together in LDS from byte 0
		for (uint32_t w = tid; w < DFL_UW; w += DFL_T) L.u[w] = 0;
		__syncthreads();
		uint32_t total;
		if (huff) {
			DflSink sk{L.u};
			al_dfl_header(sk, 18 * 8, tid, DFL_T, L.llen, L.dlen);
			uint32_t base = 18 * 8 + AL_DFL_HDRBITS;
			for (uint32_t t0 = 0; t0 < bn; t0 += DFL_T) {
				const uint32_t i = t0 + tid;
				uint32_t nbits = 0; uint64_t v = 0;
				if (i < bn && (L.sel[i >> 5] >> (i & 31) & 1)) v = al_dfl_token(mt[i], inb[i], L.lcode, L.llen, L.dcode, L.dlen, &nbits);
				uint32_t x = nbits;
				for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(x, d, 64); if (lane >= d) x += y; }
				if (lane == 63) L.wsum[wave] = x;
				__syncthreads();
				uint32_t wp = 0, tot = 0;
				for (uint32_t k = 0; k < 16; ++k) { const uint32_t s = L.wsum[k]; tot += s; if (k < wave) wp += s; }
				al_dfl_put(sk, (uint64_t)(base + wp + x - nbits), v, nbits);
				base += tot;
				__syncthreads();
			}
			if (tid == 0) al_dfl_put(sk, (uint64_t)base, L.lcode[256], L.llen[256]);
			total = 18 + comp + 8;
		} else {
			for (uint32_t i = tid; i < bn; i += DFL_T) ub[23 + i] = inb[i];
			if (tid == 0) { ub[18] = 1; ub[19] = (uint8_t)(bn & 0xff); ub[20] = (uint8_t)(bn >> 8); ub[21] = (uint8_t)(~bn & 0xff); ub[22] = (uint8_t)((~bn >> 8) & 0xff); }
			total = 18 + 5 + bn + 8;
		}
		__syncthreads();
		if (tid == 0) {
			uint8_t h[18]; al_dfl_member_header(h, total);
			for (uint32_t k = 0; k < 18; ++k) ub[k] = h[k];
			for (uint32_t k = 0; k < 4; ++k) { ub[total - 8 + k] = (uint8_t)(crc >> (8 * k)); ub[total - 4 + k] = (uint8_t)(bn >> (8 * k)); }
			sizes[b] = total; stored[b] = huff ? 0u : 1u;
		}
		__syncthreads();
		uint32_t *slot = slots + (size_t)b * DFL_UW;
		for (uint32_t w = tid; w < (total + 3) / 4; w += DFL_T) slot[w] = L.u[w];
		__syncthreads();
	}
}

// offs[b] = bytes of the members before block b, offs[nb] = all of them (one workgroup)
__global__ __launch_bounds__(1024) void k_dfl_offsets(const uint32_t *sizes, uint64_t *offs, uint32_t nb)
{
	__shared__ uint64_t ws[16];
	const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	uint64_t base = 0;
	for (uint32_t t0 = 0; t0 < nb; t0 += DFL_T) {
		const uint32_t b = t0 + tid; const uint64_t mine = b < nb ? sizes[b] : 0;
		uint64_t x = mine;
		for (uint32_t d = 1; d < 64; d <<= 1) { const uint64_t y = __shfl_up(x, d, 64); if (lane >= d) x += y; }
		if (lane == 63) ws[wave] = x;
		__syncthreads();
		uint64_t wp = 0, tot = 0;
		for (uint32_t k = 0; k < 16; ++k) { tot += ws[k]; if (k < wave) wp += ws[k]; }
		if (b < nb) offs[b] = base + wp + x - mine;
		base += tot;
		__syncthreads();
	}
	if (tid == 0) offs[nb] = base;
}
__global__ __launch_bounds__(1024) void k_dfl_pack(const uint8_t *slots, const uint32_t *sizes, const uint64_t *offs, uint8_t *packed, uint32_t nb)
{
	for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
		const uint8_t *s = slots + (size_t)b * AL_DFL_SLOT; uint8_t *d = packed + offs[b]; const uint32_t sz = sizes[b];
		for (uint32_t i = threadIdx.x; i < sz; i += DFL_T) d[i] = s[i];
	}
}

inline double dfl_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

} // namespace

struct AlDeflateDev {
	int device = 0, grid = 0;
	hipStream_t st = nullptr; hipEvent_t e0 = nullptr, e1 = nullptr;
	uint8_t *d_in = nullptr, *d_seam = nullptr, *d_slots = nullptr, *d_packed = nullptr; uint32_t *d_sizes = nullptr, *d_stored = nullptr, *d_scratch = nullptr; uint64_t *d_offs = nullptr;
	size_t cap_nb = 0, cap_in = 0;                         // blocks the output side / the input staging buffer have room for
	std::vector<uint32_t> h_stored;
};

AlDeflateDev *al_deflate_dev_open(int device)
{
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) { (void)hipGetLastError(); return nullptr; }
	device = al_env_pick_device(device, n_dev);
	AlDeflateDev *d = new AlDeflateDev(); d->device = device;
	hipDeviceProp_t pr;
	if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&pr, device) != hipSuccess || hipStreamCreateWithFlags(&d->st, hipStreamNonBlocking) != hipSuccess ||
	    hipEventCreate(&d->e0) != hipSuccess || hipEventCreate(&d->e1) != hipSuccess) { (void)hipGetLastError(); delete d; return nullptr; }
	d->grid = pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 64;
	return d;
}
static void dfl_release(AlDeflateDev *d)
{
	al_dev_free(d->d_in); al_dev_free(d->d_seam); al_dev_free(d->d_slots); al_dev_free(d->d_packed); al_dev_free(d->d_sizes); al_dev_free(d->d_stored); al_dev_free(d->d_scratch); al_dev_free(d->d_offs);
	d->d_in = d->d_seam = d->d_slots = d->d_packed = nullptr; d->cap_in = 0; d->d_sizes = d->d_stored = d->d_scratch = nullptr; d->d_offs = nullptr; d->cap_nb = 0;
}
void al_deflate_dev_close(AlDeflateDev *d)
{
	if (!d) return;
	(void)hipSetDevice(d->device);
	if (d->st) (void)hipStreamSynchronize(d->st);
	dfl_release(d);
	if (d->e0) (void)hipEventDestroy(d->e0);
	if (d->e1) (void)hipEventDestroy(d->e1);
	if (d->st) (void)hipStreamDestroy(d->st);
	delete d;
}
// room for nb blocks (need_in: also for their input, when it comes from the host); 1 when the device refuses it (nothing is held then)
static int dfl_ensure(AlDeflateDev *d, size_t nb, bool need_in)
{
	if (nb <= d->cap_nb && (!need_in || nb <= d->cap_in)) return 0;
	const bool refuse = al_env().test_deflate_nomem;      // (test switch, DESIGN.md section 8: every request is refused)
	const size_t cap = std::max(nb + nb / 4 + 1, d->cap_nb);
	const bool in = need_in || d->cap_in > 0;
	dfl_release(d);
	bool ok = !refuse;
	ok = ok && (!in || al_dev_malloc((void **)&d->d_in, cap * AL_DFL_BLOCK) == hipSuccess);
	ok = ok && al_dev_malloc((void **)&d->d_seam, AL_DFL_BLOCK) == hipSuccess;
	ok = ok && al_dev_malloc((void **)&d->d_slots, cap * AL_DFL_SLOT) == hipSuccess;
	ok = ok && al_dev_malloc((void **)&d->d_packed, cap * AL_DFL_SLOT) == hipSuccess;
	ok = ok && al_dev_malloc((void **)&d->d_sizes, cap * 4) == hipSuccess;
	ok = ok && al_dev_malloc((void **)&d->d_stored, cap * 4) == hipSuccess;
	ok = ok && al_dev_malloc((void **)&d->d_offs, (cap + 1) * 8) == hipSuccess;
	ok = ok && al_dev_malloc((void **)&d->d_scratch, (size_t)d->grid * AL_DFL_BLOCK * 4) == hipSuccess;
	if (!ok) { (void)hipGetLastError(); dfl_release(d); return 1; }
	d->cap_nb = cap; d->cap_in = in ? cap : 0;
	return 0;
}
// the three kernels over the stream s0[0, n0) + s1[0, n - n0) on stream st, between the backend's two events; *tot = bytes of the members in d_packed
static int dfl_launch(AlDeflateDev *d, hipStream_t st, const uint8_t *s0, uint64_t n0, const uint8_t *s1, uint64_t n, int level, size_t nb, uint64_t *tot, double *kernel_s)
{
	const uint32_t grid = (uint32_t)std::min<size_t>(nb, (size_t)d->grid);
	(void)hipEventRecord(d->e0, st);
	hipLaunchKernelGGL(k_deflate, dim3(grid), dim3(DFL_T), 0, st, s0, n0, s1, n, level, d->d_scratch, (uint32_t *)d->d_slots, d->d_sizes, d->d_stored, (uint32_t)nb);
	hipLaunchKernelGGL(k_dfl_offsets, dim3(1), dim3(DFL_T), 0, st, d->d_sizes, d->d_offs, (uint32_t)nb);
	hipLaunchKernelGGL(k_dfl_pack, dim3(grid), dim3(DFL_T), 0, st, d->d_slots, d->d_sizes, d->d_offs, d->d_packed, (uint32_t)nb);
	(void)hipEventRecord(d->e1, st);
	*tot = 0;
	if (hipGetLastError() != hipSuccess || hipMemcpyAsync(tot, d->d_offs + nb, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return -1;
	float ms = 0; (void)hipEventElapsedTime(&ms, d->e0, d->e1);
	if (kernel_s) *kernel_s += ms * 1e-3;
	return *tot > nb * (size_t)AL_DFL_SLOT ? -1 : 0;
}

// n host bytes as ceil(n / 0xff00) members appended to dst.  0: done; 1: the device had no room (AL_ERR_NOMEM: nothing appended, the caller compresses
// on the host); -1: a HIP call failed.  *kernel_s and *xfer_s get the seconds of the kernels (HIP events) and of the copies.
int al_deflate_dev_run(AlDeflateDev *d, const char *src, size_t n, int level, std::vector<unsigned char> &dst, size_t *n_stored, double *kernel_s, double *xfer_s)
{
	const size_t nb = (n + AL_DFL_BLOCK - 1) / AL_DFL_BLOCK;
	if (nb == 0) return 0;
	if (hipSetDevice(d->device) != hipSuccess) return -1;
	if (dfl_ensure(d, nb, true)) return 1;
	const double t0 = dfl_now();
	if (hipMemcpyAsync(d->d_in, src, n, hipMemcpyHostToDevice, d->st) != hipSuccess || hipStreamSynchronize(d->st) != hipSuccess) return -1;
	const double t1 = dfl_now();
	uint64_t tot = 0;
	if (dfl_launch(d, d->st, d->d_in, (uint64_t)n, nullptr, (uint64_t)n, level, nb, &tot, kernel_s)) return -1;
	const double t2 = dfl_now();
	const size_t at = dst.size(); dst.resize(at + tot);
	d->h_stored.resize(nb);
	if (hipMemcpyAsync(dst.data() + at, d->d_packed, tot, hipMemcpyDeviceToHost, d->st) != hipSuccess || hipMemcpyAsync(d->h_stored.data(), d->d_stored, nb * 4, hipMemcpyDeviceToHost, d->st) != hipSuccess ||
	    hipStreamSynchronize(d->st) != hipSuccess) return -1;
	const double t3 = dfl_now();
	if (n_stored) for (size_t b = 0; b < nb; ++b) *n_stored += d->h_stored[b];
	if (xfer_s) *xfer_s += (t1 - t0) + (t3 - t2);
	return 0;
}

// The device-resident form (AlBgzf::write_device): the stream's next bytes are the host's carry[0, n_carry), n_carry < 0xff00, and then d_src[0, n) in
// device memory.  Its whole blocks are compressed on st -- the first one gathered from the seam buffer, which takes the carry, and the head of d_src --,
// their members leave in pieces of `piece` bytes through the two page-locked buffers and are written to out while the next piece is copied; the
// rest, fewer bytes than a block, comes back in tail.  Needs n_carry + n >= 0xff00.  0 / 1 (no room) / -1 as al_deflate_dev_run.
int al_deflate_dev_run_resident(AlDeflateDev *d, hipStream_t st, const char *carry, size_t n_carry, const char *d_src, size_t n, int level, char *const ring[2], size_t piece, hipEvent_t const ev[2],
                                FILE *out, std::vector<char> &tail, size_t *n_stored, double *kernel_s, double *xfer_s)
{
	const size_t total = n_carry + n, nb = total / AL_DFL_BLOCK, nt = total - nb * AL_DFL_BLOCK;
	if (nb == 0 || n_carry >= AL_DFL_BLOCK || nt > n) return -1;
	if (hipSetDevice(d->device) != hipSuccess) return -1;
	if (dfl_ensure(d, nb, false)) return 1;
	const double t0 = dfl_now();
	if (n_carry && (hipMemcpyAsync(d->d_seam, carry, n_carry, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) return -1;
	const double t1 = dfl_now();
	uint64_t tot = 0;
	if (dfl_launch(d, st, d->d_seam, (uint64_t)n_carry, (const uint8_t *)d_src, (uint64_t)(nb * AL_DFL_BLOCK), level, nb, &tot, kernel_s)) return -1;
	const double t2 = dfl_now();
	const uint64_t np = (tot + piece - 1) / piece;
	auto fetch = [&](uint64_t c) { return hipMemcpyAsync(ring[c & 1], d->d_packed + c * piece, (size_t)std::min<uint64_t>(piece, tot - c * piece), hipMemcpyDeviceToHost, st) == hipSuccess && hipEventRecord(ev[c & 1], st) == hipSuccess; };
	if (np && !fetch(0)) return -1;
	for (uint64_t c = 0; c < np; ++c) {
		if (c + 1 < np && !fetch(c + 1)) return -1;
		if (hipEventSynchronize(ev[c & 1]) != hipSuccess) return -1;
		const size_t m = (size_t)std::min<uint64_t>(piece, tot - c * piece);
		if (fwrite(ring[c & 1], 1, m, out) != m) return -1;
	}
	tail.resize(nt); d->h_stored.resize(nb);
	if ((nt && hipMemcpyAsync(tail.data(), d_src + (n - nt), nt, hipMemcpyDeviceToHost, st) != hipSuccess) || hipMemcpyAsync(d->h_stored.data(), d->d_stored, nb * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
	    hipStreamSynchronize(st) != hipSuccess) return -1;
	const double t3 = dfl_now();
	if (n_stored) for (size_t b = 0; b < nb; ++b) *n_stored += d->h_stored[b];
	if (xfer_s) *xfer_s += (t1 - t0) + (t3 - t2);     // (the drain's copies overlap the writes: this is their wall time, writes included)
	return 0;
}

// the same members from the host twin, on n_threads workers
int al_deflate_host_run(const char *src, size_t n, int level, int n_threads, std::vector<unsigned char> &dst, size_t *n_stored)
{
	const size_t nb = (n + AL_DFL_BLOCK - 1) / AL_DFL_BLOCK;
	if (nb == 0) return 0;
	std::vector<std::vector<unsigned char>> blk(nb); std::vector<int> st(nb, 0);
	al_parallel_for(n_threads > 1 ? n_threads : 1, nb, [&](size_t lo, size_t hi, int) {
		for (size_t b = lo; b < hi; ++b) {
			blk[b].resize(AL_DFL_SLOT);
			const size_t o = b * AL_DFL_BLOCK;
			blk[b].resize(al_deflate_block_host((const uint8_t *)src + o, (uint32_t)std::min<size_t>(AL_DFL_BLOCK, n - o), level, blk[b].data(), &st[b]));
		}
	});
	for (size_t b = 0; b < nb; ++b) { dst.insert(dst.end(), blk[b].begin(), blk[b].end()); if (n_stored) *n_stored += (size_t)st[b]; }
	return 0;
}

// test tap (airlift_amd/capi.py): a whole BGZF file from AlBgzf with the device backend, the stream handed over in calls of `piece` bytes that lie in
// DEVICE memory (AlBgzf::write_device, as the stream driver's writer does with a batch); mix != 0: every second call goes through write() from the
// host instead, so that carries of both kinds meet.  The members leave through two page-locked buffers of ring_bytes.
extern "C" int al_dbg_bgzf_stream_dev(int device, const void *src, size_t n, size_t piece, int mix, size_t ring_bytes, int level, void *dst, size_t cap, size_t *out_n)
{
	char *mem = nullptr; size_t len = 0;
	FILE *f = open_memstream(&mem, &len);
	if (!f) return -1;
	int rc = 0;
	hipStream_t st = nullptr; hipEvent_t ev[2] = {nullptr, nullptr}; char *ring[2] = {nullptr, nullptr}; char *d_src = nullptr;
	if (piece == 0) piece = n ? n : 1;
	if (ring_bytes == 0) ring_bytes = 1 << 20;
	{
		AlBgzf z(f, (level & 0xff) | 0x100, 2, device);
		z.cap = (size_t)3 * AL_DFL_BLOCK;
		int n_dev = 0;
		if (hipGetDeviceCount(&n_dev) != hipSuccess || hipSetDevice(device < 0 ? 0 : device) != hipSuccess || hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess ||
		    hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess || hipHostMalloc((void **)&ring[0], ring_bytes, hipHostMallocDefault) != hipSuccess ||
		    hipHostMalloc((void **)&ring[1], ring_bytes, hipHostMallocDefault) != hipSuccess || al_dev_malloc((void **)&d_src, piece + 1) != hipSuccess) rc = -1;
		size_t k = 0;
		for (size_t o = 0; o < n && rc == 0; o += piece, ++k) {
			const size_t m = std::min(piece, n - o);
			int r = 1;
			if (!(mix && (k & 1))) {
				if (hipMemcpyAsync(d_src, (const char *)src + o, m, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { rc = -1; break; }
				r = z.write_device(d_src, m, st, ring, ring_bytes, ev);
			}
			if (r < 0) rc = -1; else if (r > 0) rc = z.write((const char *)src + o, m);
		}
		if (rc == 0) rc = z.finish();
		if (rc == 0 && n >= 4 * (size_t)AL_DFL_BLOCK && piece >= 2 * (size_t)AL_DFL_BLOCK && z.n_resident == 0) rc = -5;      // (the path under test was not taken)
	}
	if (st) (void)hipStreamSynchronize(st);
	if (d_src) al_dev_free(d_src);
	for (int i = 0; i < 2; ++i) { if (ring[i]) (void)hipHostFree(ring[i]); if (ev[i]) (void)hipEventDestroy(ev[i]); }
	if (st) (void)hipStreamDestroy(st);
	fclose(f);
	if (rc == 0 && len <= cap) { memcpy(dst, mem, len); *out_n = len; } else if (rc == 0) rc = -2;
	free(mem);
	return rc;
}

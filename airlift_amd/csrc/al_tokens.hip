// al_tokens.hip -- tokens --gaps-bed: the tokens of a batch set up on the GPU from the table of BED regions (the function: al_dev_tokens.h).
//
//   k_tok_setup   lane per token of the batch: its row by binary search in first_tok, its k, the first base of its window in the index's own S4 and its
//                 fragment hash (the row's X31 state continued over the digits of k * S, then the Wang terms); it also writes the per-read arrays a token
//                 batch has (rd_off, rd_len, frag_first, mini_off: affine in the token's index)
//   k_make_windows (al_runtime.hip) then cuts the reads from S4 at those starts.
// Per batch the host sends the kernel's arguments; no per-token array is built or copied.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "al_internal.h"
#include "al_device.h"
#include "al_runtime.h"
#include "al_dev_tokens.h"

struct TokOut { uint64_t *start; uint32_t *frag_hash; uint64_t *rd_off; uint32_t *rd_len, *frag_first; uint64_t *mini_off; };   // rd_off == nullptr (the tap): start and frag_hash only

__global__ void __launch_bounds__(256)
k_tok_setup(AlTokTab T, uint64_t t0, uint32_t n_tok, int R, int S, int seed, uint32_t wpr, uint32_t mper, TokOut O)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i > n_tok) return;
	if (O.rd_off) {                                                      // entry n_tok: the end of the last read
		O.rd_off[i] = (uint64_t)i * wpr; O.mini_off[i] = (uint64_t)i * mper; O.frag_first[i] = i; O.rd_len[i] = i < n_tok ? (uint32_t)R : 0u;
		if (i == n_tok) O.frag_hash[i] = 0;
	}
	if (i == n_tok) return;
	uint32_t row, hash; uint64_t start;
	al_tok_setup(T, t0 + i, R, S, seed, &row, &start, &hash);
	O.start[i] = start; O.frag_hash[i] = hash;
}

#define TOK_CHECK(x) AL_HIP_CHECK_AS("tokens", x)

struct AlTokDev {
	int device = 0; uint32_t n_rows = 0; uint64_t n_tok = 0;
	DevBuf<uint64_t> first_tok, src; DevBuf<uint32_t> h_prefix;
	hipEvent_t ev[2] = {}; float ms = 0;
	AlTokTab tab() const { return AlTokTab{first_tok.p, src.p, h_prefix.p, n_rows}; }
};

AlTokDev *al_tokdev_open(int device, const uint64_t *first_tok, const uint64_t *src, const uint32_t *h_prefix, uint32_t n_rows)
{
	AlTokDev *T = new AlTokDev();
	T->device = device < 0 ? 0 : device; T->n_rows = n_rows; T->n_tok = first_tok[n_rows];
	auto init = [&]() -> int {
		TOK_CHECK(hipSetDevice(T->device));
		for (hipEvent_t &e : T->ev) TOK_CHECK(hipEventCreate(&e));
		if (T->first_tok.ensure((size_t)n_rows + 1) || T->src.ensure((size_t)n_rows + 1) || T->h_prefix.ensure((size_t)n_rows + 1)) return -1;
		TOK_CHECK(hipMemcpy(T->first_tok.p, first_tok, ((size_t)n_rows + 1) * 8, hipMemcpyHostToDevice));
		if (n_rows) { TOK_CHECK(hipMemcpy(T->src.p, src, (size_t)n_rows * 8, hipMemcpyHostToDevice)); TOK_CHECK(hipMemcpy(T->h_prefix.p, h_prefix, (size_t)n_rows * 4, hipMemcpyHostToDevice)); }
		return 0;
	};
	if (init()) { al_tokdev_close(T); return nullptr; }
	return T;
}
void al_tokdev_close(AlTokDev *T)
{
	if (!T) return;
	(void)hipSetDevice(T->device); (void)hipDeviceSynchronize();
	T->first_tok.release(); T->src.release(); T->h_prefix.release();
	for (hipEvent_t &e : T->ev) if (e) (void)hipEventDestroy(e);
	delete T;
}
float al_tokdev_ms(const AlTokDev *T) { return T ? T->ms : 0.f; }

// the packed reference of a context's index copied to the host: a device-built index keeps none (the SAM sink prints the tokens' bases from it)
int al_tokdev_fetch_s4(al_ctx_t *c, std::vector<uint32_t> &S4)
{
	if (!c || !c->di.S4) return -1;
	AL_HIP_CHECK(hipSetDevice(c->device));
	const size_t nw = (size_t)((c->mi->tot_len + 7) / 8);
	S4.assign(nw + 8, 0);
	if (nw) AL_HIP_CHECK(hipMemcpy(S4.data(), c->di.S4, nw * 4, hipMemcpyDeviceToHost));
	return 0;
}

int al_batch_upload_tokens(al_ctx_t *c, const AlTokDev *T, uint64_t t0, int n_tok, int read_len, int skip, bool host_mirrors)
{
	if (!c || !T || n_tok < 0 || read_len <= 0 || skip < 1 || T->device != c->device) return -1;
	if (t0 + (uint64_t)n_tok > T->n_tok) { fprintf(stderr, "[airlift] al_batch_upload_tokens: tokens [%llu, %llu) leave the table of %llu\n", (unsigned long long)t0, (unsigned long long)(t0 + (uint64_t)n_tok), (unsigned long long)T->n_tok); return -2; }
	AL_HIP_CHECK(hipSetDevice(c->device));
	int rc = al_windows_prepare(c, n_tok, read_len);
	if (rc) return rc;
	c->h_rd_off.clear(); c->h_mini_off.clear(); c->h_frag_first.clear(); c->h_frag_hash.clear();   // (no host mirror of what the kernel writes)
	if (host_mirrors) { c->h_rd_len.assign((size_t)n_tok + 1, (uint32_t)read_len); c->h_rd_len[n_tok] = 0; c->h_flip.assign(n_tok, 0); }
	else { c->h_rd_len.clear(); c->h_flip.clear(); }
	const int k = c->mi->k; const uint32_t wpr = (uint32_t)((read_len + 7) / 8 + 1), mper = (uint32_t)(read_len >= k ? read_len - k + 1 : 0) + 1u;
	hipStream_t s = c->stream; AlTokDev *Tm = const_cast<AlTokDev *>(T);
	AL_HIP_CHECK(hipEventRecord(Tm->ev[0], s));
	hipLaunchKernelGGL(k_tok_setup, dim3(((unsigned)n_tok + 1 + 255) / 256), dim3(256), 0, s, T->tab(), t0, (uint32_t)n_tok, read_len, skip, c->opt.seed, wpr, mper,
	                   TokOut{c->tmp_u64b.p, c->frag_hash.p, c->rd_off.p, c->rd_len.p, c->frag_first.p, c->mini_off.p});
	AL_HIP_CHECK(hipGetLastError());
	AL_HIP_CHECK(hipEventRecord(Tm->ev[1], s));
	if ((rc = al_windows_cut(c, c->di.S4, n_tok, read_len)) != 0) return rc;
	AL_HIP_CHECK(hipStreamSynchronize(s));
	float ms = 0; AL_HIP_CHECK(hipEventElapsedTime(&ms, Tm->ev[0], Tm->ev[1])); Tm->ms += ms;
	return 0;
}

// ---- test taps: a caller-given table, no index, no mapping -------------------------------------------------------------------------------------------------
static int tap_table(uint32_t n_rows, const char *names, size_t names_len, const uint32_t *len, int R, int S, uint64_t t0, uint64_t n,
                     std::vector<uint64_t> &first_tok, std::vector<uint32_t> &h_prefix)
{
	if (R <= 0 || S < 1 || (n_rows && (!names || !len))) return -1;
	std::vector<std::string> heads; heads.reserve(n_rows);
	for (size_t at = 0; heads.size() < n_rows; ) {                        // n_rows NUL-terminated names inside names[0, names_len)
		const void *z = at < names_len ? memchr(names + at, 0, names_len - at) : nullptr;
		if (!z) return -1;
		heads.emplace_back(names + at, (const char *)z - (names + at)); at = (size_t)((const char *)z - names) + 1;
	}
	al_tok_table(heads, len, R, S, first_tok, h_prefix);
	return t0 + n > first_tok[n_rows] || t0 + n < t0 ? -1 : 0;
}
extern "C" int al_dbg_tokens_table_host(uint32_t n_rows, const char *names, size_t names_len, const uint64_t *src, const uint32_t *len, int read_size, int skip, int seed,
                                        uint64_t t0, uint64_t n, uint64_t *o_start, uint32_t *o_hash, uint64_t *o_first_tok, uint32_t *o_h_prefix)
{
	std::vector<uint64_t> first_tok; std::vector<uint32_t> h_prefix;
	if ((n && (!o_start || !o_hash)) || (n_rows && !src) || tap_table(n_rows, names, names_len, len, read_size, skip, t0, n, first_tok, h_prefix)) return -1;
	if (o_first_tok) memcpy(o_first_tok, first_tok.data(), first_tok.size() * 8);
	if (o_h_prefix && n_rows) memcpy(o_h_prefix, h_prefix.data(), h_prefix.size() * 4);
	al_tok_setup_host(AlTokTab{first_tok.data(), src, h_prefix.data(), n_rows}, t0, n, read_size, skip, seed, o_start, o_hash);
	return 0;
}
extern "C" int al_dbg_tokens_table(uint32_t n_rows, const char *names, size_t names_len, const uint64_t *src, const uint32_t *len, int read_size, int skip, int seed,
                                   uint64_t t0, uint64_t n, uint64_t *o_start, uint32_t *o_hash, uint64_t *o_first_tok, uint32_t *o_h_prefix)
{
	std::vector<uint64_t> first_tok; std::vector<uint32_t> h_prefix;
	if ((n && (!o_start || !o_hash)) || (n_rows && !src) || n >= (1ull << 31) || tap_table(n_rows, names, names_len, len, read_size, skip, t0, n, first_tok, h_prefix)) return -1;
	if (o_first_tok) memcpy(o_first_tok, first_tok.data(), first_tok.size() * 8);
	if (o_h_prefix && n_rows) memcpy(o_h_prefix, h_prefix.data(), h_prefix.size() * 4);
	if (n == 0) return 0;
	int dev = 0;
	if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); fprintf(stderr, "[airlift] al_dbg_tokens_table: no HIP device\n"); return -2; }
	AlTokDev *T = al_tokdev_open(dev, first_tok.data(), src, h_prefix.data(), n_rows);
	if (!T) return -2;
	DevBuf<uint64_t> d_start; DevBuf<uint32_t> d_hash;
	auto run = [&]() -> int {
		if (d_start.ensure(n) || d_hash.ensure(n)) return -1;
		hipLaunchKernelGGL(k_tok_setup, dim3(((unsigned)n + 1 + 255) / 256), dim3(256), 0, 0, T->tab(), t0, (uint32_t)n, read_size, skip, seed, 0u, 0u,
		                   TokOut{d_start.p, d_hash.p, nullptr, nullptr, nullptr, nullptr});
		TOK_CHECK(hipGetLastError());
		TOK_CHECK(hipMemcpy(o_start, d_start.p, n * 8, hipMemcpyDeviceToHost));
		TOK_CHECK(hipMemcpy(o_hash, d_hash.p, n * 4, hipMemcpyDeviceToHost));
		return 0;
	};
	const int rc = run();
	(void)hipDeviceSynchronize();
	d_start.release(); d_hash.release();
	al_tokdev_close(T);
	return rc;
}

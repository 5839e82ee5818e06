// al_regions.hip -- tokens --regions-bed / --merged-bed: the gap regions merged on the GPU, beside the records (the function: al_dev_regions.h).
//
//   k_reg_intervals  lane per token of the resident batch: the records the SAM writer would print, read where al_batch_run left them (out_off / out), each
//                    appended as {group, contig rank, rs, re} to the device list; a wavefront reserves its slots with one atomic
//   AlRegions::fold  the list becomes its regions in place: the fold of al_fold.h under AlRegFold (merge sort, max-scan, head sum, k_fold_compact), plain rule;
//                    k_fold_compact leaves the new count where k_reg_intervals adds to it
//   k_reg_zero_group the groups of the per-gap regions set to 0: the merge across all gaps is the same fold once more
// The list is folded whenever it holds more than AL_REG_FOLD_CAP intervals, and once at the end; only the regions are copied to the host.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "al_internal.h"
#include "al_device.h"
#include "al_runtime.h"
#include "al_stream.h"
#include "al_dev_regions.h"
#include "al_fold.h"

__global__ void __launch_bounds__(256)
k_reg_intervals(const uint64_t *__restrict__ out_off, const AlReg *__restrict__ out, uint32_t n_tok, uint32_t tok0, const uint32_t *__restrict__ g_first, const uint32_t *__restrict__ g_id, uint32_t n_g,
                const uint32_t *__restrict__ rank_of, uint32_t n_seq, int no_print_2nd, AlRegIv *__restrict__ list, uint64_t cap, unsigned long long *__restrict__ cnt /* [0] intervals held, [1] refused */)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
	uint64_t k0 = 0, k1 = 0; uint32_t c = 0;
	if (i < n_tok) {
		k0 = out_off[i]; k1 = out_off[i + 1];
		for (uint64_t k = k0; k < k1; ++k) c += al_reg_printed(out[k].id, out[k].parent, no_print_2nd != 0) ? 1u : 0u;
	}
	// slots of the wavefront: inclusive sum of c over the lanes, one atomic by the last lane, the base to every lane (no lane has left: the block is whole wavefronts)
	uint32_t incl = c;
	for (int d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(incl, d, 64); if ((int)lane >= d) incl += v; }
	const uint32_t total = __shfl(incl, 63, 64);
	if (total == 0) return;                                              // (uniform in the wavefront)
	unsigned long long base = 0;
	if (lane == 63) base = atomicAdd(cnt, (unsigned long long)total);
	base = __shfl(base, 63, 64);
	if (base + total > cap) { if (lane == 63) atomicAdd(cnt + 1, (unsigned long long)total); return; }   // never happens (the host sized the list for every record); never silent
	if (c == 0) return;
	// the token's group: the last run of the batch's table that starts at or before it
	const uint32_t tok = tok0 + i;
	uint32_t lo = 0, hi = n_g;
	while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (g_first[mid] <= tok) lo = mid; else hi = mid; }
	const uint32_t group = g_id[lo];
	uint64_t o = base + incl - c;
	for (uint64_t k = k0; k < k1; ++k) {
		const AlReg *r = out + k;
		if (!al_reg_printed(r->id, r->parent, no_print_2nd != 0)) continue;
		const uint32_t rid = (uint32_t)r->rid;
		if (rid >= n_seq) { atomicAdd(cnt + 1, 1ull); continue; }
		list[o++] = AlRegIv{group, rank_of[rid], (uint32_t)r->rs, (uint32_t)r->re};
	}
}

__global__ void __launch_bounds__(256)
k_reg_zero_group(AlRegIv *__restrict__ list, uint32_t n)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) list[i].group = 0;
}

#define REG_CHECK(x) AL_HIP_CHECK_AS("regions", x)

struct AlRegions {
	int device = 0; bool no_print_2nd = true; uint32_t n_seq = 0, n_g = 0;
	uint64_t n = 0;                                                      // intervals the list holds
	DevBuf<AlRegIv> list, sorted; DevBuf<uint64_t> run_max; DevBuf<uint32_t> idx, rank_of, g_first, g_id; DevBuf<uint8_t> tmp; DevBuf<unsigned long long> cnt;
	hipEvent_t ev[2] = {};
	AlRegionsStat st = {0, 0, 0, 0, 0, 0};
	int fold();
	int room(uint64_t more);
};

AlRegions *al_regions_open(int device, const uint32_t *rank_of, uint32_t n_seq, bool no_print_2nd)
{
	AlRegions *R = new AlRegions();
	R->device = device < 0 ? 0 : device; R->no_print_2nd = no_print_2nd; R->n_seq = n_seq;
	auto init = [&]() -> int {
		REG_CHECK(hipSetDevice(R->device));
		for (hipEvent_t &e : R->ev) REG_CHECK(hipEventCreate(&e));
		if (R->cnt.ensure(2) || R->rank_of.ensure((size_t)n_seq + 1)) return -1;
		REG_CHECK(hipMemset(R->cnt.p, 0, 16));
		if (n_seq) REG_CHECK(hipMemcpy(R->rank_of.p, rank_of, (size_t)n_seq * 4, hipMemcpyHostToDevice));
		R->st.bytes_h2d += (uint64_t)n_seq * 4;
		return 0;
	};
	if (init()) { al_regions_close(R); return nullptr; }
	return R;
}
void al_regions_close(AlRegions *R)
{
	if (!R) return;
	(void)hipSetDevice(R->device); (void)hipDeviceSynchronize();
	R->list.release(); R->sorted.release(); R->run_max.release(); R->idx.release(); R->rank_of.release(); R->g_first.release(); R->g_id.release(); R->tmp.release(); R->cnt.release();
	for (hipEvent_t &e : R->ev) if (e) (void)hipEventDestroy(e);
	delete R;
}
void al_regions_stat(const AlRegions *R, AlRegionsStat *st) { *st = R->st; }
void al_regions_device_list(const AlRegions *R, const AlRegIv **list, uint64_t *n, int *device) { *list = R->list.p; *n = R->n; *device = R->device; }

// the list becomes its regions, in place (n: their number)
int AlRegions::fold()
{
	if (n == 0) return 0;
	if (n >= (1ull << 31)) { fprintf(stderr, "[airlift] regions: %llu intervals are more than one fold takes\n", (unsigned long long)n); return -1; }
	const uint32_t m = (uint32_t)n; hipStream_t s = 0;
	auto nomem = [&]() { fprintf(stderr, "[airlift] regions: no device memory to fold %u intervals\n", m); return AL_ERR_NOMEM; };
	if (sorted.ensure(m) || run_max.ensure(m) || idx.ensure((size_t)m + 1)) return nomem();
	REG_CHECK(hipEventRecord(ev[0], s));
	int r = al_fold_enqueue<AlRegFold>("regions", list.p, m, m, false, list.p, cnt.p, sorted.p, run_max.p, idx.p, tmp, s);
	if (r) return r == AL_ERR_NOMEM ? nomem() : r;
	REG_CHECK(hipEventRecord(ev[1], s));
	uint32_t h = 0;
	if ((r = al_fold_count("regions", idx.p, m, s, &h)) != 0) return r;
	float ms = 0; REG_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
	st.ms_fold += ms; ++st.n_fold; st.bytes_d2h += 4;
	n = h;
	return 0;
}

// room for `more` further intervals behind the n held: grown with its contents kept; when the device refuses, the list is folded first
int AlRegions::room(uint64_t more)
{
	if (n + more <= list.cap) return 0;
	if (list.ensure(n + more, true) == 0) return 0;
	fprintf(stderr, "[airlift] regions: folding %llu intervals to make room for %llu more\n", (unsigned long long)n, (unsigned long long)more);
	const int r = fold();
	if (r) return r;
	if (n + more <= list.cap || list.ensure(n + more, true) == 0) return 0;
	fprintf(stderr, "[airlift] regions: no device memory for %llu intervals\n", (unsigned long long)(n + more));
	return AL_ERR_NOMEM;
}

int al_regions_groups(AlRegions *R, const uint32_t *first, const uint32_t *group, uint32_t n)
{
	if (!R || n == 0 || first[0] != 0) return -1;
	REG_CHECK(hipSetDevice(R->device));
	if (R->g_first.ensure(n) || R->g_id.ensure(n)) return -1;
	REG_CHECK(hipMemcpy(R->g_first.p, first, (size_t)n * 4, hipMemcpyHostToDevice));
	REG_CHECK(hipMemcpy(R->g_id.p, group, (size_t)n * 4, hipMemcpyHostToDevice));
	R->n_g = n; R->st.bytes_h2d += (uint64_t)n * 8;
	return 0;
}

int al_regions_take(AlRegions *R, al_ctx_s *c, uint32_t tok0)
{
	if (!R || !c || R->n_g == 0) return -1;
	REG_CHECK(hipSetDevice(R->device));
	if (c->n_reads == 0) return 0;
	AlDevResult D;
	const int rc = al_align_result(c, &D);
	if (rc) return rc;
	if (D.out_total == 0) return 0;
	int r = R->room(D.out_total);                                        // every record of the batch has a slot, printed or not
	if (r) return r;
	hipStream_t s = 0;
	const uint32_t n_tok = (uint32_t)c->n_reads;
	REG_CHECK(hipEventRecord(R->ev[0], s));
	hipLaunchKernelGGL(k_reg_intervals, dim3((n_tok + 255) / 256), dim3(256), 0, s, D.out_off, D.out, n_tok, tok0, (const uint32_t *)R->g_first.p, (const uint32_t *)R->g_id.p, R->n_g,
	                   (const uint32_t *)R->rank_of.p, R->n_seq, R->no_print_2nd ? 1 : 0, R->list.p, (uint64_t)R->list.cap, R->cnt.p);
	REG_CHECK(hipGetLastError());
	REG_CHECK(hipEventRecord(R->ev[1], s));
	unsigned long long h[2] = {0, 0};
	REG_CHECK(hipMemcpy(h, R->cnt.p, 16, hipMemcpyDeviceToHost));
	float ms = 0; REG_CHECK(hipEventElapsedTime(&ms, R->ev[0], R->ev[1]));
	R->st.ms_intervals += ms; R->st.bytes_d2h += 16;
	if (h[1] || h[0] < R->n || h[0] > R->n + D.out_total) { fprintf(stderr, "[airlift] regions: k_reg_intervals refused %llu records (%llu held, %llu before the batch of %llu)\n", h[1], h[0], (unsigned long long)R->n, (unsigned long long)D.out_total); return -1; }
	R->st.n_raw += h[0] - R->n; R->n = h[0];
	return R->n > AL_REG_FOLD_CAP ? R->fold() : 0;
}

int al_regions_append(AlRegions *R, const AlRegIv *iv, uint64_t n, bool fold)
{
	if (!R) return -1;
	REG_CHECK(hipSetDevice(R->device));
	if (n) {
		const int r = R->room(n);
		if (r) return r;
		const unsigned long long h = R->n + n;
		REG_CHECK(hipMemcpy(R->list.p + R->n, iv, n * sizeof(AlRegIv), hipMemcpyHostToDevice));
		REG_CHECK(hipMemcpy(R->cnt.p, &h, 8, hipMemcpyHostToDevice));
		R->n = h; R->st.n_raw += n; R->st.bytes_h2d += n * sizeof(AlRegIv);
	}
	return fold ? R->fold() : 0;
}

int al_regions_finish(AlRegions *R, std::vector<AlRegIv> *per_gap, std::vector<AlRegIv> *merged)
{
	if (!R) return -1;
	REG_CHECK(hipSetDevice(R->device));
	int r = R->fold();
	if (r) return r;
	auto fetch = [&](std::vector<AlRegIv> &v) -> int {
		v.resize(R->n);
		if (R->n) REG_CHECK(hipMemcpy(v.data(), R->list.p, R->n * sizeof(AlRegIv), hipMemcpyDeviceToHost));
		R->st.bytes_d2h += R->n * sizeof(AlRegIv);
		return 0;
	};
	if (per_gap && fetch(*per_gap)) return -1;
	if (!merged) return 0;
	if (R->n) {
		hipLaunchKernelGGL(k_reg_zero_group, dim3(((uint32_t)R->n + 255) / 256), dim3(256), 0, 0, R->list.p, (uint32_t)R->n);
		REG_CHECK(hipGetLastError());
		if ((r = R->fold()) != 0) return r;
	}
	return fetch(*merged);
}

// ---- test taps ---------------------------------------------------------------------------------------------------------------------------------------------------
static void tap_pack(uint64_t n, const uint32_t *g, const uint32_t *k, const uint32_t *s, const uint32_t *e, std::vector<AlRegIv> &v)
{
	v.resize(n);
	for (uint64_t i = 0; i < n; ++i) v[i] = AlRegIv{g[i], k[i], s[i], e[i]};
}
static void tap_unpack(const std::vector<AlRegIv> &v, uint32_t *g, uint32_t *k, uint32_t *s, uint32_t *e, uint64_t *n_out)
{
	for (size_t i = 0; i < v.size(); ++i) { g[i] = v[i].group; k[i] = v[i].rank; s[i] = v[i].start; e[i] = v[i].end; }
	*n_out = v.size();
}
extern "C" int al_dbg_regions_merge_host(uint64_t n, const uint32_t *group, const uint32_t *rank, const uint32_t *start, const uint32_t *end, uint64_t chunk, int per_gap,
                                         uint32_t *o_group, uint32_t *o_rank, uint32_t *o_start, uint32_t *o_end, uint64_t *n_out)
{
	if (!n_out || (n && (!group || !rank || !start || !end || !o_group || !o_rank || !o_start || !o_end))) return -1;
	std::vector<AlRegIv> in, v; tap_pack(n, group, rank, start, end, in);
	al_regions_chunked_host(in.data(), n, chunk, per_gap != 0, v);
	tap_unpack(v, o_group, o_rank, o_start, o_end, n_out);
	return 0;
}
extern "C" int al_dbg_regions_merge(uint64_t n, const uint32_t *group, const uint32_t *rank, const uint32_t *start, const uint32_t *end, uint64_t chunk, int per_gap,
                                    uint32_t *o_group, uint32_t *o_rank, uint32_t *o_start, uint32_t *o_end, uint64_t *n_out)
{
	if (!n_out || (n && (!group || !rank || !start || !end || !o_group || !o_rank || !o_start || !o_end))) return -1;
	std::vector<AlRegIv> in, v; tap_pack(n, group, rank, start, end, in);
	int dev = 0;
	if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); fprintf(stderr, "[airlift] al_dbg_regions_merge: no HIP device\n"); return -2; }
	AlRegions *R = al_regions_open(dev, nullptr, 0, true);
	if (!R) return -2;
	int rc = 0;
	for (uint64_t at = 0; at < n && rc == 0; ) {
		const uint64_t m = chunk ? std::min(chunk, n - at) : n;
		rc = al_regions_append(R, in.data() + at, m, chunk != 0); at += m;
	}
	if (rc == 0) rc = per_gap ? al_regions_finish(R, &v, nullptr) : al_regions_finish(R, nullptr, &v);
	al_regions_close(R);
	if (rc == 0) tap_unpack(v, o_group, o_rank, o_start, o_end, n_out);
	return rc;
}

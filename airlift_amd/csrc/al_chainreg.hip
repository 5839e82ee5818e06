// al_chainreg.hip -- chain-beds / tokens --chain: the chain file's region logic on the GPU (the function: al_dev_chainreg.h).
//
//   (scan)          segmented sum of size + dt over the lines of every chain (al_chn_sum_op): T[i] = tStart + the sum before line i
//   k_chn_expand    lane per line: its padded gap, its padded block (retired step) and its block as it is (constant rows), each as {slot, start, end, index}
//   k_chn_expand_m  lane per merged region (retired step): the row padded, its slot from the row itself (uploaded) or from its rank (the run's device list)
//   ChainRegDev::fold  the fold of al_fold.h under AlChnFold (merge sort by (slot, start, index), max-scan over the slot's prefix -- see FORM OF THE MERGE in
//                   the header --, head sum strict or not, k_fold_compact): the elements of a slot that is some become the regions reg[]
//   k_chn_invert    lane per region: its leading hole into row 2j, and the slot's hole count (one atomic per hole)
//   k_chn_tail      lane per region: the tail of the last region of a slot that has a hole, into row 2j + 1
//   k_chn_gather    the rows that are some, in order, to the front (exclusive sum of their flags)
// Only result rows are copied to the host.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include "al_internal.h"
#include "al_device.h"
#include "al_runtime.h"
#include "al_dev_chainreg.h"
#include "al_fold.h"

// T of line i from the inclusive sums
__device__ __forceinline__ uint32_t chn_T(const AlChnLine &l, const uint64_t *__restrict__ tsum, const uint32_t *__restrict__ c_tstart, uint32_t i)
{
	return c_tstart[l.chain] + (uint32_t)tsum[i] - (l.size + l.dt);
}

__global__ void __launch_bounds__(256)
k_chn_expand(const AlChnLine *__restrict__ line, const uint64_t *__restrict__ tsum, uint32_t n, const uint32_t *__restrict__ c_slot, const uint32_t *__restrict__ c_tstart, uint32_t n_chain,
             const uint32_t *__restrict__ L, uint32_t n_slot, const uint32_t *__restrict__ rslot_of, const uint32_t *__restrict__ RL, uint32_t n_rslot, uint32_t p_gap, uint32_t p_blk, uint32_t idx0,
             AlChnIv *__restrict__ gap /* [n] or null */, AlChnIv *__restrict__ blk /* [n], element idx0 + i of the retired step's list, or null */, AlChnIv *__restrict__ raw /* [n] or null */,
             unsigned long long *__restrict__ bad)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const AlChnLine l = line[i];
	if (l.chain >= n_chain) { atomicAdd(bad, 1ull); return; }              // never happens (the host made the table); never silent, never out of bounds
	const uint32_t s = c_slot[l.chain];
	if (s >= n_slot) { atomicAdd(bad, 1ull); return; }
	const uint32_t T = chn_T(l, tsum, c_tstart, i);
	if (gap) gap[i] = al_chn_gap(l, T, s, p_gap, L[s], i);
	if (raw) raw[i] = al_chn_block(l, T, s, 0, L[s], i);
	if (blk) {
		const uint32_t rs = rslot_of[s];
		if (rs >= n_rslot) { atomicAdd(bad, 1ull); return; }
		AlChnIv v = al_chn_block(l, T, rs, 0, RL[rs], idx0 + i);
		al_chn_pad(v.start, v.end, p_blk, RL[rs], &v.start, &v.end);
		blk[i] = v;
	}
}
__global__ void __launch_bounds__(256)
k_chn_expand_m(const AlRegIv *__restrict__ M, uint32_t n_m, const uint32_t *__restrict__ rank_rslot /* null: the rank is the slot */, uint32_t n_rank, const uint32_t *__restrict__ RL, uint32_t n_rslot,
               uint32_t p, AlChnIv *__restrict__ out, unsigned long long *__restrict__ bad)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_m) return;
	const AlRegIv m = M[i];
	AlChnIv v{AL_CHN_NONE, 0, 0, i};                                      // (a refused row sorts behind every slot; the host sees `bad` and gives up)
	uint32_t rs = m.rank;
	if (rank_rslot) rs = m.rank < n_rank ? rank_rslot[m.rank] : AL_CHN_NONE;
	if (rs >= n_rslot || m.start > m.end || m.start >= RL[rs]) atomicAdd(bad, 1ull);
	else { v.slot = rs; al_chn_pad(m.start, m.end, p, RL[rs], &v.start, &v.end); }
	out[i] = v;
}

struct ChnLessIdx { __host__ __device__ bool operator()(const AlChnIv &a, const AlChnIv &b) const { return al_chn_less_idx(a, b); } };
struct ChnSumOp { __host__ __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return al_chn_sum_op(a, b); } };
struct ChnSumIn {
	const AlChnLine *l;
	__host__ __device__ uint64_t operator()(uint32_t i) const { return al_chn_sum_elem(i == 0 || l[i - 1].chain != l[i].chain, l[i].size + l[i].dt); }
};
struct ChnSomeIn {             // row i is some (i == n: the total)
	const AlChnIv *r; uint32_t n;
	__host__ __device__ uint32_t operator()(uint32_t i) const { return i < n && r[i].slot != AL_CHN_NONE ? 1u : 0u; }
};

__global__ void __launch_bounds__(256)
k_chn_invert(const AlChnIv *__restrict__ reg, uint32_t k, AlChnIv *__restrict__ rows /* [2k] */, uint32_t *__restrict__ holes, uint32_t n_rslot)
{
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= k) return;
	const AlChnIv h = al_chn_hole(reg, j);
	rows[2 * (size_t)j] = h;
	if (h.slot != AL_CHN_NONE && h.slot < n_rslot) atomicAdd(holes + h.slot, 1u);
}
__global__ void __launch_bounds__(256)
k_chn_tail(const AlChnIv *__restrict__ reg, uint32_t k, AlChnIv *__restrict__ rows, const uint32_t *__restrict__ holes, const uint32_t *__restrict__ RL, uint32_t n_rslot)
{
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= k) return;
	const uint32_t s = reg[j].slot;
	AlChnIv t{AL_CHN_NONE, 0, 0, 0};
	if (s < n_rslot) t = al_chn_tail(reg, k, j, holes[s], RL[s]);
	rows[2 * (size_t)j + 1] = t;
}
__global__ void __launch_bounds__(256)
k_chn_gather(const AlChnIv *__restrict__ rows, const uint32_t *__restrict__ idx, uint32_t n, AlChnIv *__restrict__ out)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	if (idx[i + 1] != idx[i]) out[idx[i]] = rows[i];                      // (idx has n + 1 entries, idx[n] <= n rows are written)
}

#define CHN_CHECK(x) AL_HIP_CHECK_AS("chainreg", x)
#define CHN_LAUNCH(kern, n, ...) kern<<<dim3(((uint32_t)(n) + 255) / 256), dim3(256), 0, s>>>(__VA_ARGS__)

namespace {
struct ChainRegDev {
	DevBuf<AlChnLine> line; DevBuf<uint64_t> tsum, run_max; DevBuf<uint32_t> c_slot, c_tstart, L, rslot_of, RL, rank_rslot, idx, holes;
	DevBuf<AlChnIv> a, b, sorted, reg, rows; DevBuf<AlRegIv> m; DevBuf<uint8_t> tmp; DevBuf<unsigned long long> bad;
	hipEvent_t ev[2] = {}; hipStream_t s = 0; AlChnStat st;
	~ChainRegDev()
	{
		(void)hipDeviceSynchronize();
		line.release(); tsum.release(); run_max.release(); c_slot.release(); c_tstart.release(); L.release(); rslot_of.release(); RL.release(); rank_rslot.release(); idx.release(); holes.release();
		a.release(); b.release(); sorted.release(); reg.release(); rows.release(); m.release(); tmp.release(); bad.release();
		for (hipEvent_t &e : ev) if (e) (void)hipEventDestroy(e);
	}
	template <class T> int up(DevBuf<T> &d, const T *h, size_t n)
	{
		if (d.ensure(n + 1)) return AL_ERR_NOMEM;
		if (n) CHN_CHECK(hipMemcpy(d.p, h, n * sizeof(T), hipMemcpyHostToDevice));
		st.bytes_h2d += n * sizeof(T);
		return 0;
	}
	template <class T> int down(std::vector<T> &h, const T *d, size_t n)
	{
		h.resize(n);
		if (n) CHN_CHECK(hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
		st.bytes_d2h += n * sizeof(T);
		return 0;
	}
	// idx[0, n] = exclusive sum of in(0..n); *total = idx[n]
	template <class In> int sum_flags(In in, uint32_t n, uint32_t *total)
	{
		if (idx.ensure((size_t)n + 2)) return AL_ERR_NOMEM;
		auto it = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint32_t>(0u), in);
		const int r = al_prim_run(tmp, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, it, idx.p, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), s); }, "chainreg");
		if (r) return r;
		CHN_CHECK(hipMemcpyAsync(total, idx.p + n, 4, hipMemcpyDeviceToHost, s));
		CHN_CHECK(hipStreamSynchronize(s));
		st.bytes_d2h += 4;
		return 0;
	}
	template <class Less> int sort(const AlChnIv *in, uint32_t n, Less less)
	{
		if (sorted.ensure(n)) return AL_ERR_NOMEM;
		return al_prim_run(tmp, [&](void *t, size_t &b) { return rocprim::merge_sort(t, b, in, sorted.p, (size_t)n, less, s); }, "chainreg");
	}
	// the n_all elements of `in` become their regions reg[0, *k); only the first n of the sorted list are of a slot that is some (the others sort behind them)
	int fold(const AlChnIv *in, uint32_t n_all, uint32_t n, bool strict, uint32_t *k)
	{
		*k = 0;
		if (n == 0) return 0;
		if (sorted.ensure(n_all) || run_max.ensure(n) || idx.ensure((size_t)n + 1) || reg.ensure(n)) return AL_ERR_NOMEM;
		const int r = al_fold_enqueue<AlChnFold>("chainreg", in, n_all, n, strict, reg.p, nullptr, sorted.p, run_max.p, idx.p, tmp, s);
		if (r) return r;
		st.bytes_d2h += 4;
		return al_fold_count("chainreg", idx.p, n, s, k);
	}
	int run(const AlChnIn &in, int R, int E, std::vector<AlChnIv> *gaps, std::vector<AlChnIv> *constant, std::vector<AlChnIv> *retired);
};

int ChainRegDev::run(const AlChnIn &in, int R, int E, std::vector<AlChnIv> *gaps, std::vector<AlChnIv> *constant, std::vector<AlChnIv> *retired)
{
	const uint64_t n_u = in.n + in.n_m;
	if (in.n >= 0x7ffffff0ull || n_u >= 0x7ffffff0ull) { fprintf(stderr, "[airlift] chainreg: %llu lines and %llu merged regions are more than one run takes\n", (unsigned long long)in.n, (unsigned long long)in.n_m); return -1; }
	const uint32_t n = (uint32_t)in.n, n_m = (uint32_t)in.n_m;
	for (hipEvent_t &e : ev) CHN_CHECK(hipEventCreate(&e));
	int r;
	if (bad.ensure(2)) return AL_ERR_NOMEM;
	CHN_CHECK(hipMemset(bad.p, 0, 16));
	if ((r = up(line, in.line, n)) || (r = up(c_slot, in.c_slot, in.n_chain)) || (r = up(c_tstart, in.c_tstart, in.n_chain)) || (r = up(L, in.L, in.n_slot))) return r;
	if (retired) {
		if ((r = up(rslot_of, in.rslot_of, in.n_slot)) || (r = up(RL, in.RL, in.n_rslot))) return r;
		if (in.dev_M) { if ((r = up(rank_rslot, in.rank_rslot, in.n_rank))) return r; }
		else {                                                           // uploaded in the device list's layout: the rank is the slot
			std::vector<AlRegIv> hm(n_m);
			for (uint32_t i = 0; i < n_m; ++i) hm[i] = AlRegIv{0, in.M[i].slot, in.M[i].start, in.M[i].end};
			if ((r = up(m, hm.data(), n_m))) return r;
		}
		if (holes.ensure((size_t)in.n_rslot + 1)) return AL_ERR_NOMEM;
		CHN_CHECK(hipMemset(holes.p, 0, ((size_t)in.n_rslot + 1) * 4));
	}
	if (tsum.ensure((size_t)n + 1) || (gaps && a.ensure((size_t)n + 1)) || (retired && b.ensure(n_u + 1)) || (constant && rows.ensure((size_t)n + 1))) return AL_ERR_NOMEM;
	CHN_CHECK(hipEventRecord(ev[0], s));
	if (n) {
		auto in_sum = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint32_t>(0u), ChnSumIn{line.p});
		if ((r = al_prim_run(tmp, [&](void *t, size_t &b) { return rocprim::inclusive_scan(t, b, in_sum, tsum.p, (size_t)n, ChnSumOp(), s); }, "chainreg")) != 0) return r;
		CHN_LAUNCH(k_chn_expand, n, (const AlChnLine *)line.p, (const uint64_t *)tsum.p, n, (const uint32_t *)c_slot.p, (const uint32_t *)c_tstart.p, in.n_chain,
		                   (const uint32_t *)L.p, in.n_slot, (const uint32_t *)rslot_of.p, (const uint32_t *)RL.p, in.n_rslot, (uint32_t)(R + (E > 0 ? E : 0)), (uint32_t)R, n_m,
		                   gaps ? a.p : nullptr, retired ? b.p + n_m : nullptr, constant ? rows.p : nullptr, bad.p);
		CHN_CHECK(hipGetLastError());
	}
	if (retired && n_m) {
		CHN_LAUNCH(k_chn_expand_m, n_m, in.dev_M ? in.dev_M : (const AlRegIv *)m.p, n_m, in.dev_M ? (const uint32_t *)rank_rslot.p : nullptr, in.n_rank, (const uint32_t *)RL.p, in.n_rslot,
		                   (uint32_t)R, b.p, bad.p);
		CHN_CHECK(hipGetLastError());
	}
	unsigned long long h_bad = 0;
	CHN_CHECK(hipMemcpy(&h_bad, bad.p, 8, hipMemcpyDeviceToHost));
	if (h_bad) { fprintf(stderr, "[airlift] chainreg: %llu lines or merged regions lie outside their tables or contigs\n", h_bad); return -1; }
	uint32_t k = 0;
	if (gaps) {        // the 1-field lines' elements (slot AL_CHN_NONE) sort behind every slot: the first n_three elements are folded
		uint32_t n_three = 0;
		for (uint32_t i = 0; i < n; ++i) n_three += in.line[i].three ? 1u : 0u;
		if ((r = fold(a.p, n, n_three, true, &k)) != 0) return r;
		if ((r = down(*gaps, (const AlChnIv *)reg.p, k)) != 0) return r;
	}
	if (constant) {
		if (n && (r = sort(rows.p, n, ChnLessIdx())) != 0) return r;
		if ((r = down(*constant, (const AlChnIv *)sorted.p, n)) != 0) return r;
	}
	if (retired) {
		uint32_t n_rows = 0;
		if ((r = fold(b.p, (uint32_t)n_u, (uint32_t)n_u, false, &k)) != 0) return r;
		if (k) {
			if (rows.ensure(2 * (size_t)k + 1) || a.ensure(2 * (size_t)k + 1)) return AL_ERR_NOMEM;
			CHN_LAUNCH(k_chn_invert, k, (const AlChnIv *)reg.p, k, rows.p, holes.p, in.n_rslot);
			CHN_CHECK(hipGetLastError());
			CHN_LAUNCH(k_chn_tail, k, (const AlChnIv *)reg.p, k, rows.p, (const uint32_t *)holes.p, (const uint32_t *)RL.p, in.n_rslot);
			CHN_CHECK(hipGetLastError());
			if ((r = sum_flags(ChnSomeIn{rows.p, 2 * k}, 2 * k, &n_rows)) != 0) return r;
			if (n_rows > 2 * k) { fprintf(stderr, "[airlift] chainreg: %u regions left %u rows\n", k, n_rows); return -1; }
			CHN_LAUNCH(k_chn_gather, 2 * k, (const AlChnIv *)rows.p, (const uint32_t *)idx.p, 2 * k, a.p);
			CHN_CHECK(hipGetLastError());
		}
		if ((r = down(*retired, (const AlChnIv *)a.p, n_rows)) != 0) return r;
	}
	CHN_CHECK(hipEventRecord(ev[1], s));
	CHN_CHECK(hipEventSynchronize(ev[1]));
	float ms = 0; CHN_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
	st.ms_kernels = ms;
	return 0;
}
}  // namespace

int al_chainreg_device(int device, const AlChnIn &in, int R, int E, std::vector<AlChnIv> *gaps, std::vector<AlChnIv> *constant, std::vector<AlChnIv> *retired, AlChnStat *st)
{
	if (hipSetDevice(device < 0 ? 0 : device) != hipSuccess) { (void)hipGetLastError(); fprintf(stderr, "[airlift] chainreg: no HIP device %d\n", device < 0 ? 0 : device); return -2; }
	ChainRegDev D;
	const int rc = D.run(in, R, E, gaps, constant, retired);
	if (st) *st = D.st;
	return rc;
}

// ---- chain-beds ---------------------------------------------------------------------------------------------------------------------------------------------------
extern "C" int al_chain_beds(const char *chain_fn, int read_size, int max_errors, const char *merged_fn, FILE *gaps, FILE *constant, FILE *retired, unsigned flags, int device)
{
	if (!chain_fn || (!gaps && !constant && !retired)) { fprintf(stderr, "[ERROR] airlift: al_chain_beds needs a chain file and at least one output\n"); return -1; }
	if (read_size < 1 || read_size > (1 << 30)) { fprintf(stderr, "[ERROR] airlift: al_chain_beds: the read size must be positive\n"); return -1; }
	if (gaps && (max_errors < 0 || max_errors > (1 << 30))) { fprintf(stderr, "[ERROR] airlift: al_chain_beds: the gaps rows need the maximum number of errors (--max-errors)\n"); return -1; }
	if (retired && !merged_fn) { fprintf(stderr, "[ERROR] airlift: al_chain_beds: the retired rows need the merged regions (--merged-in)\n"); return -1; }
	AlChnTab tab; AlChnRet ret; std::string err;
	if (al_chn_parse(chain_fn, tab, err) != 0 || (retired && al_chn_parse_merged(merged_fn, tab, ret, err) != 0)) { fprintf(stderr, "[ERROR] airlift: %s\n", err.c_str()); return -1; }
	AlChnIn in = tab.in();
	if (retired) al_chn_ret_in(ret, in);
	std::vector<AlChnIv> g, c, r;
	if (flags & AL_CHAIN_HOST) {
		const auto t0 = std::chrono::steady_clock::now();
		al_chainreg_host(in, read_size, max_errors, gaps ? &g : nullptr, constant ? &c : nullptr, retired ? &r : nullptr);
		if (al_env().timing) fprintf(stderr, "[airlift] chainreg: %zu lines, %zu merged regions; %zu gaps rows, %zu constant, %zu retired; host twin %.3f ms\n",
		                             tab.line.size(), ret.M.size(), g.size(), c.size(), r.size(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
	} else {
		AlChnStat st;
		const int rc = al_chainreg_device(device, in, read_size, max_errors, gaps ? &g : nullptr, constant ? &c : nullptr, retired ? &r : nullptr, &st);
		if (rc != 0) return rc;
		if (al_env().timing) fprintf(stderr, "[airlift] chainreg: %zu lines, %zu merged regions; %zu gaps rows, %zu constant, %zu retired; kernels %.3f ms; bytes to the device %llu, from the device %llu\n",
		                             tab.line.size(), ret.M.size(), g.size(), c.size(), r.size(), st.ms_kernels, (unsigned long long)st.bytes_h2d, (unsigned long long)st.bytes_d2h);
	}
	std::string text;
	auto put = [&](FILE *f, const std::vector<AlChnIv> &v, const std::vector<std::string> &names) -> int {
		if (!f) return 0;
		text.clear(); al_chn_bed(text, v.data(), v.size(), names);
		return fwrite(text.data(), 1, text.size(), f) != text.size() || fflush(f) == EOF ? -3 : 0;
	};
	if (put(gaps, g, tab.name) || put(constant, c, tab.name) || put(retired, r, ret.name)) return -3;
	return 0;
}

// ---- test taps ---------------------------------------------------------------------------------------------------------------------------------------------------
static int chn_tap(bool dev, uint64_t n, const uint32_t *chain, const uint32_t *size, const uint32_t *dt, const uint32_t *three, uint32_t n_chain, const uint32_t *c_slot, const uint32_t *c_tstart,
                   uint32_t n_slot, const uint32_t *L, uint64_t n_m, const uint32_t *m_slot, const uint32_t *m_start, const uint32_t *m_end, uint32_t n_rslot, const uint32_t *rslot_of, const uint32_t *RL,
                   int R, int E, uint32_t *o_gaps, uint64_t *n_gaps, uint32_t *o_constant, uint64_t *n_constant, uint32_t *o_retired, uint64_t *n_retired)
{
	if (R < 1 || R > (1 << 30) || E > (1 << 30) || (n && (!chain || !size || !dt || !three)) || (n_chain && (!c_slot || !c_tstart)) || (n_slot && !L) || (n_m && (!m_slot || !m_start || !m_end))) return -1;
	if ((n_gaps && (!o_gaps || E < 0)) || (n_constant && !o_constant) || (n_retired && (!o_retired || (n_slot && !rslot_of) || (n_rslot && !RL)))) return -1;
	std::vector<AlChnLine> line(n); std::vector<AlChnIv> M(n_m);
	for (uint64_t i = 0; i < n; ++i) line[i] = AlChnLine{chain[i], size[i], dt[i], three[i] ? 1u : 0u};
	for (uint64_t i = 0; i < n_m; ++i) M[i] = AlChnIv{m_slot[i], m_start[i], m_end[i], 0};
	AlChnIn in; in.n = n; in.line = line.data(); in.n_chain = n_chain; in.c_slot = c_slot; in.c_tstart = c_tstart; in.n_slot = n_slot; in.L = L;
	if (n_retired) { in.n_m = n_m; in.M = M.data(); in.n_rslot = n_rslot; in.rslot_of = rslot_of; in.RL = RL; }
	const char *why = al_chn_in_bad(in, n_retired != nullptr);
	if (why) { fprintf(stderr, "[airlift] al_dbg_chainreg: %s\n", why); return -1; }
	std::vector<AlChnIv> g, c, r;
	if (dev) {
		int d = 0;
		if (hipGetDevice(&d) != hipSuccess) { (void)hipGetLastError(); fprintf(stderr, "[airlift] al_dbg_chainreg: no HIP device\n"); return -2; }
		const int rc = al_chainreg_device(d, in, R, E, n_gaps ? &g : nullptr, n_constant ? &c : nullptr, n_retired ? &r : nullptr, nullptr);
		if (rc != 0) return rc;
	} else al_chainreg_host(in, R, E, n_gaps ? &g : nullptr, n_constant ? &c : nullptr, n_retired ? &r : nullptr);
	auto out = [](const std::vector<AlChnIv> &v, uint32_t *o, uint64_t *cnt) { if (!cnt) return; for (size_t i = 0; i < v.size(); ++i) { o[3 * i] = v[i].slot; o[3 * i + 1] = v[i].start; o[3 * i + 2] = v[i].end; } *cnt = v.size(); };
	out(g, o_gaps, n_gaps); out(c, o_constant, n_constant); out(r, o_retired, n_retired);
	return 0;
}
extern "C" int al_dbg_chainreg(uint64_t n, const uint32_t *chain, const uint32_t *size, const uint32_t *dt, const uint32_t *three, uint32_t n_chain, const uint32_t *c_slot, const uint32_t *c_tstart,
                               uint32_t n_slot, const uint32_t *L, uint64_t n_m, const uint32_t *m_slot, const uint32_t *m_start, const uint32_t *m_end, uint32_t n_rslot, const uint32_t *rslot_of, const uint32_t *RL,
                               int R, int E, uint32_t *o_gaps, uint64_t *n_gaps, uint32_t *o_constant, uint64_t *n_constant, uint32_t *o_retired, uint64_t *n_retired)
{
	return chn_tap(true, n, chain, size, dt, three, n_chain, c_slot, c_tstart, n_slot, L, n_m, m_slot, m_start, m_end, n_rslot, rslot_of, RL, R, E, o_gaps, n_gaps, o_constant, n_constant, o_retired, n_retired);
}
extern "C" int al_dbg_chainreg_host(uint64_t n, const uint32_t *chain, const uint32_t *size, const uint32_t *dt, const uint32_t *three, uint32_t n_chain, const uint32_t *c_slot, const uint32_t *c_tstart,
                                    uint32_t n_slot, const uint32_t *L, uint64_t n_m, const uint32_t *m_slot, const uint32_t *m_start, const uint32_t *m_end, uint32_t n_rslot, const uint32_t *rslot_of, const uint32_t *RL,
                                    int R, int E, uint32_t *o_gaps, uint64_t *n_gaps, uint32_t *o_constant, uint64_t *n_constant, uint32_t *o_retired, uint64_t *n_retired)
{
	return chn_tap(false, n, chain, size, dt, three, n_chain, c_slot, c_tstart, n_slot, L, n_m, m_slot, m_start, m_end, n_rslot, rslot_of, RL, R, E, o_gaps, n_gaps, o_constant, n_constant, o_retired, n_retired);
}

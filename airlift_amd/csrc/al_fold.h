// al_fold.h -- the fold of al_dev_fold.h on the device, for the .hip files: one merge sort, the max-scan, the head sum and one compact kernel, over the
// caller's buffers on the caller's stream.
//   (merge sort)    the list under Tr::less: one rocPRIM merge sort of the 16-byte elements
//   (scan)          segmented inclusive max-scan of `end` (al_fold_scan_op) -- the running maximum every later element is compared with
//   (scan)          exclusive sum of the head flags (al_fold_head, strict or not): every element's region number, and their count
//   k_fold_compact  one element per region: the head writes Tr::head's fields, the region's last element its running maximum
#pragma once
#include "al_prim.h"
#include "al_dev_fold.h"

template <class Tr> struct AlFoldLess { __host__ __device__ bool operator()(const typename Tr::Elem &a, const typename Tr::Elem &b) const { return Tr::less(a, b); } };
struct AlFoldMaxOp { __host__ __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return al_fold_scan_op(a, b); } };
template <class Tr> struct AlFoldMaxIn {             // element i of the max-scan's input
	const typename Tr::Elem *s;
	__host__ __device__ uint64_t operator()(uint32_t i) const { return al_fold_scan_elem(i == 0 || !Tr::same_seg(s[i - 1], s[i]), s[i].end); }
};
template <class Tr> struct AlFoldHeadIn {            // element i of the head sum's input (i == n: the sum's last element, the total)
	const typename Tr::Elem *s; const uint64_t *m; uint32_t n; bool strict;
	__host__ __device__ uint32_t operator()(uint32_t i) const { return i < n && al_fold_head<Tr>(s, m, i, strict) ? 1u : 0u; }
};

template <class Tr> __global__ void __launch_bounds__(256)
k_fold_compact(const typename Tr::Elem *__restrict__ s, const uint64_t *__restrict__ m, const uint32_t *__restrict__ idx, uint32_t n, typename Tr::Elem *__restrict__ reg, unsigned long long *__restrict__ cnt /* or null */)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint32_t k = idx[i], k_next = idx[i + 1];                      // idx[i + 1] - idx[i]: 1 when i is a head; idx has n + 1 entries, idx[n] = the number of regions
	const bool head = k_next != k, last = i + 1 == n || idx[i + 2] != k_next;
	const uint32_t r = head ? k : k - 1;                                  // the region i belongs to (element 0 is a head, so k >= 1 where i is none, and r < idx[n] <= n)
	if (head) Tr::head(reg[r], s[i], r);
	if (last) reg[r].end = (uint32_t)m[i];
	if (cnt && i + 1 == n) cnt[0] = idx[n];
}

// Enqueued on s: the n_all elements of `in` sorted into sorted[n_all], and the first n of them (1 <= n <= n_all; the others sort behind them) folded to
// their regions out[0, idx[n]) through run_max[n] and idx[n + 1] -- `out` has room for n and may be `in`; cnt[0], unless cnt is null, becomes their number.
// 0, AL_ERR_NOMEM or -1 (al_prim_run).
template <class Tr>
static inline int al_fold_enqueue(const char *tag, const typename Tr::Elem *in, uint32_t n_all, uint32_t n, bool strict, typename Tr::Elem *out, unsigned long long *cnt,
                                  typename Tr::Elem *sorted, uint64_t *run_max, uint32_t *idx, DevBuf<uint8_t> &tmp, hipStream_t s, int line = __builtin_LINE(), const char *file = __builtin_FILE())
{
	typedef typename Tr::Elem E;
	int r = al_prim_run(tmp, [&](void *t, size_t &b) { return rocprim::merge_sort(t, b, in, sorted, (size_t)n_all, AlFoldLess<Tr>(), s); }, tag, line, file);
	if (r) return r;
	auto in_max = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint32_t>(0u), AlFoldMaxIn<Tr>{sorted});
	if ((r = al_prim_run(tmp, [&](void *t, size_t &b) { return rocprim::inclusive_scan(t, b, in_max, run_max, (size_t)n, AlFoldMaxOp(), s); }, tag, line, file)) != 0) return r;
	auto in_head = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint32_t>(0u), AlFoldHeadIn<Tr>{sorted, run_max, n, strict});
	if ((r = al_prim_run(tmp, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, in_head, idx, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), s); }, tag, line, file)) != 0) return r;
	hipLaunchKernelGGL(k_fold_compact<Tr>, dim3((n + 255) / 256), dim3(256), 0, s, (const E *)sorted, (const uint64_t *)run_max, (const uint32_t *)idx, n, out, cnt);
	const hipError_t e = hipGetLastError();
	if (e != hipSuccess) { fprintf(stderr, "[airlift] %s: k_fold_compact: %s\n", tag, hipGetErrorString(e)); return -1; }
	return 0;
}
// ... and, s synchronised, the number of regions it left: 4 bytes from the device.  -1 unless 1 <= *k <= n.
static inline int al_fold_count(const char *tag, const uint32_t *idx, uint32_t n, hipStream_t s, uint32_t *k)
{
	*k = 0;
	hipError_t e = hipMemcpyAsync(k, idx + n, 4, hipMemcpyDeviceToHost, s);
	if (e == hipSuccess) e = hipStreamSynchronize(s);
	if (e != hipSuccess) { fprintf(stderr, "[airlift] %s: the fold of %u intervals: %s\n", tag, n, hipGetErrorString(e)); return -1; }
	if (*k == 0 || *k > n) { fprintf(stderr, "[airlift] %s: the fold of %u intervals left %u\n", tag, n, *k); return -1; }
	return 0;
}

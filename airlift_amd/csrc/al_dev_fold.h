// al_dev_fold.h -- the interval fold that al_dev_regions.h and al_dev_chainreg.h share: a list of intervals becomes its regions.  Written once for both
// sides: the pieces are compiled for the device (al_fold.h) and for the CPU (the twin at the end of this file).
//
// An element is 16 bytes of four uint32_t, two of them `start` and `end`.  A traits type Tr says what the others mean:
//   Tr::Elem            the element
//   Tr::less(a, b)      the order the list is sorted in: the segment first, then start, then a tie-break
//   Tr::same_seg(a, b)  a and b may share a region
//   Tr::head(r, h, k)   region number k takes its fields from its head h (all but `end`)
//  1. Running maximum.  In sorted order M[i] = the largest end of the elements of i's segment up to and including i: an inclusive scan with
//     al_fold_scan_op over (segment starts here, end) pairs, (f1, m1) + (f2, m2) = (f1 | f2, f2 ? m2 : max(m1, m2)), which is associative.
//  2. Heads.  Element i starts a region when it starts a segment or start[i] > M[i - 1] (strict: start[i] >= M[i - 1]): M, not the previous end, is
//     compared, so a nested interval does not shorten the region.
//  3. Regions.  Region k = the fields of its head and the M of its last element.
// The twin compares with the end of the current REGION, the device with the maximum over the segment's PREFIX; why these are the same number where the
// rule is strict too is FORM OF THE MERGE in al_dev_chainreg.h.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "al_dev_deflate.h"       // AL_DHD
#if defined(__HIPCC__)
#define AL_DHD_M static __host__ __device__       // a static member of a traits type
#else
#define AL_DHD_M static
#endif

// a scan element: bit 32 = a segment starts at (or inside) what the element covers, low word = the running maximum of `end` since then
AL_DHD uint64_t al_fold_scan_elem(bool seg_start, uint32_t end) { return (seg_start ? 1ull << 32 : 0ull) | end; }
AL_DHD uint64_t al_fold_scan_op(uint64_t a, uint64_t b)
{
	const uint32_t ma = (uint32_t)a, mb = (uint32_t)b;
	return ((a | b) & (1ull << 32)) | ((b >> 32 & 1) ? mb : (ma > mb ? ma : mb));
}
// element i of the sorted list s[] (running maxima m[] of its predecessors) starts a region
template <class Tr> AL_DHD bool al_fold_head(const typename Tr::Elem *s, const uint64_t *m, uint64_t i, bool strict)
{
	if (i == 0 || !Tr::same_seg(s[i - 1], s[i])) return true;
	const uint32_t mx = (uint32_t)m[i - 1];
	return strict ? s[i].start >= mx : s[i].start > mx;
}

// ---- the host twin ---------------------------------------------------------------------------------------------------------------------------------------------
// v becomes its regions, as `sort-bed | mergeBed` and the scripts' interval_merge make them: sorted, then one pass in which the end compared is the region's
template <class Tr> static inline void al_fold_host(std::vector<typename Tr::Elem> &v, bool strict)
{
	typedef typename Tr::Elem E;
	std::sort(v.begin(), v.end(), [](const E &a, const E &b) { return Tr::less(a, b); });
	size_t k = 0;
	for (size_t i = 0; i < v.size(); ++i) {
		if (k && Tr::same_seg(v[k - 1], v[i]) && (strict ? v[i].start < v[k - 1].end : v[i].start <= v[k - 1].end)) { if (v[i].end > v[k - 1].end) v[k - 1].end = v[i].end; }
		else v[k++] = v[i];
	}
	v.resize(k);
}

// al_dev_regions.h -- the gap regions of `tokens --regions-bed / --merged-bed` as ONE function of a set of intervals, written once for both sides: the
// pieces below are compiled for the device (k_reg_intervals and the fold, al_regions.hip) and for the CPU (the twin at the end of this file, which
// evaluates the same function serially).  The twin is what the kernels are tested against, and what tests/csrc/regions_main.cpp runs under the sanitizers.
//
// THE FUNCTION.  Input: intervals {group, rank, start, end} -- [start, end) on the contig whose NAME has rank `rank` in byte order, found by a token of
// gap sequence `group` (the index of its '>' entry in GAPS.fa).  Output: the intervals of every (group, rank) merged as `sort-bed | mergeBed` (distance 0)
// merges them, in the order (group, rank, start, end): the fold of al_dev_fold.h under AlRegFold, with the plain rule --
//
//  1. Order.  al_reg_less: (group, rank, start, end), all unsigned.
//  2. Segments.  al_reg_same_seg: one per (group, rank).
//  3. Heads.  Element i starts a region when it starts a segment or start[i] > M[i - 1]: a book-ended interval (start == M) joins.
//  4. Regions.  Region k = {group, rank, start of its head, M of its last element}.
//
// Merging is idempotent and merging merged regions with further intervals equals merging all the raw intervals, so the list may be folded (replaced by
// its regions) at any time: the device does so whenever the raw list passes AL_REG_FOLD_CAP.  The merge across all gaps is the same fold over the per-gap
// regions with every group set to 0.
#pragma once
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include <string>
#include <vector>
#include "al_dev_fold.h"

#define AL_REG_FOLD_CAP (1u << 21)   // intervals the device list may hold before it is folded in place: a run holds at most this many plus one batch's

struct alignas(16) AlRegIv { uint32_t group, rank, start, end; };

AL_DHD bool al_reg_less(const AlRegIv &a, const AlRegIv &b)
{
	if (a.group != b.group) return a.group < b.group;
	if (a.rank != b.rank) return a.rank < b.rank;
	if (a.start != b.start) return a.start < b.start;
	return a.end < b.end;
}
AL_DHD bool al_reg_same_seg(const AlRegIv &a, const AlRegIv &b) { return a.group == b.group && a.rank == b.rank; }
struct AlRegFold {
	typedef AlRegIv Elem;
	AL_DHD_M bool less(const AlRegIv &a, const AlRegIv &b) { return al_reg_less(a, b); }
	AL_DHD_M bool same_seg(const AlRegIv &a, const AlRegIv &b) { return al_reg_same_seg(a, b); }
	AL_DHD_M void head(AlRegIv &r, const AlRegIv &h, uint32_t) { r.group = h.group; r.rank = h.rank; r.start = h.start; }
};
// the record the SAM writer prints for a hit (write_batch, al_pipeline.cpp): every hit, without the secondary ones (id != parent) under AL_F_NO_PRINT_2ND
AL_DHD bool al_reg_printed(int32_t id, int32_t parent, bool no_print_2nd) { return !(no_print_2nd && id != parent); }

// Contig names in the order of sort-bed / sortBed (bytes, unsigned): rank_of[rid] and the name of every rank.  Contigs of one name share a rank.
static inline void al_regions_ranks(const std::vector<std::string> &names, std::vector<uint32_t> &rank_of, std::vector<std::string> &name_of)
{
	std::vector<uint32_t> ord(names.size());
	for (size_t i = 0; i < ord.size(); ++i) ord[i] = (uint32_t)i;
	auto cmp = [&](uint32_t a, uint32_t b) {
		const std::string &x = names[a], &y = names[b];
		const int c = memcmp(x.data(), y.data(), std::min(x.size(), y.size()));
		return c ? c < 0 : x.size() < y.size();
	};
	std::stable_sort(ord.begin(), ord.end(), cmp);
	rank_of.assign(names.size(), 0); name_of.clear();
	for (size_t i = 0; i < ord.size(); ++i) {
		if (i == 0 || names[ord[i]] != names[ord[i - 1]]) name_of.push_back(names[ord[i]]);
		rank_of[ord[i]] = (uint32_t)name_of.size() - 1;
	}
}

// BED text of regions in their order: "contig\tstart\tend\n"
static inline void al_regions_bed(std::string &o, const AlRegIv *v, size_t n, const std::vector<std::string> &name_of)
{
	char num[32];
	for (size_t i = 0; i < n; ++i) {
		o += name_of[v[i].rank];
		o.append(num, (size_t)snprintf(num, sizeof(num), "\t%u\t%u\n", v[i].start, v[i].end));
	}
}

// ---- the host twin ---------------------------------------------------------------------------------------------------------------------------------------------
// The taps' schedule on the twin (al_fold_host): the intervals are appended `chunk` at a time (0: all at once) with a fold after every append, then folded once more;
// !per_gap: the fold with the groups zeroed follows.
static inline void al_regions_chunked_host(const AlRegIv *in, uint64_t n, uint64_t chunk, bool per_gap, std::vector<AlRegIv> &v)
{
	v.clear();
	for (uint64_t at = 0; at < n; ) {
		const uint64_t m = chunk ? std::min(chunk, n - at) : n;
		v.insert(v.end(), in + at, in + at + m); at += m;
		if (chunk) al_fold_host<AlRegFold>(v, false);
	}
	al_fold_host<AlRegFold>(v, false);
	if (!per_gap) { for (AlRegIv &x : v) x.group = 0; al_fold_host<AlRegFold>(v, false); }
}

// ---- the device list (al_regions.hip) ------------------------------------------------------------------------------------------------------------------------
// One per run: the intervals of every batch appended where the records lie, folded in place whenever more than AL_REG_FOLD_CAP are held.
struct AlRegions;
struct al_ctx_s;
AlRegions *al_regions_open(int device, const uint32_t *rank_of, uint32_t n_seq, bool no_print_2nd);
// the groups of the batch's tokens: tokens [first[j], first[j + 1]) (first[0] == 0, the last run ends with the batch) belong to group[j]
int  al_regions_groups(AlRegions *R, const uint32_t *first, const uint32_t *group, uint32_t n);
// after al_batch_run: the intervals of the resident batch's records; its token i is token tok0 + i of the batch al_regions_groups described
int  al_regions_take(AlRegions *R, al_ctx_s *c, uint32_t tok0);
int  al_regions_append(AlRegions *R, const AlRegIv *iv, uint64_t n, bool fold);     // (the tap) caller-given intervals
// the last fold; per_gap / merged (either may be null) receive the regions
int  al_regions_finish(AlRegions *R, std::vector<AlRegIv> *per_gap, std::vector<AlRegIv> *merged);
// after al_regions_finish with `merged`: where the merged regions {0, rank, start, end} lie on the device (tokens --chain reads them there), and the device
void al_regions_device_list(const AlRegions *R, const AlRegIv **list, uint64_t *n, int *device);
struct AlRegionsStat { double ms_intervals, ms_fold; uint64_t n_raw, n_fold, bytes_h2d, bytes_d2h; };
void al_regions_stat(const AlRegions *R, AlRegionsStat *st);
void al_regions_close(AlRegions *R);

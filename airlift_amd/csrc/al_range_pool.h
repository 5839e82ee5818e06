// al_range_pool.h -- the free list of the device memory reserve (al_devmem.cpp): chunks of an address space cut into page-aligned ranges, best fit,
// free neighbours coalesced within a chunk.  Host code only: no HIP include, no lock, no global, and the addresses are numbers it never dereferences,
// so tests/csrc/range_pool_main.cpp runs it on made-up chunks without a GPU (make san-range-pool, tests/test_range_pool_san_cpu.py).
// The caller (DevPool) holds the mutex around every call.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <map>
#include <utility>
#include <vector>

struct AlRangePool {
	static constexpr size_t ALIGN = 4096;
	static size_t round_up(size_t bytes) { return (bytes + ALIGN - 1) / ALIGN * ALIGN; }

	std::vector<std::pair<uintptr_t, size_t>> regions;            // the chunks: (base, bytes), in the order they were added
	size_t in_use = 0, peak = 0, n_served = 0;

	void add_chunk(uintptr_t base, size_t bytes) { regions.emplace_back(base, bytes); free_[base] = bytes; }

	// The smallest free block that holds round_up(bytes), the lowest address among equal sizes; what is left of the block stays free.
	// 0 = not served: no block fits, or bytes == 0 (a range of no pages would share its address with the next one handed out).
	uintptr_t alloc(size_t bytes)
	{
		const size_t need = round_up(bytes);
		if (need == 0) return 0;
		auto best = free_.end();
		for (auto it = free_.begin(); it != free_.end(); ++it) if (it->second >= need && (best == free_.end() || it->second < best->second)) best = it;
		if (best == free_.end()) return 0;
		const uintptr_t p = best->first; const size_t sz = best->second;
		free_.erase(best);
		if (sz > need) free_[p + need] = sz - need;
		used_[p] = need; in_use += need; if (in_use > peak) peak = in_use; ++n_served;
		return p;
	}

	// false: p is not the start of a handed-out range (the caller's range came from elsewhere)
	bool free(uintptr_t p)
	{
		auto it = used_.find(p);
		if (it == used_.end()) return false;
		size_t sz = it->second;
		used_.erase(it); in_use -= sz;
		const auto *rg = region_of(p);
		auto nx = free_.find(p + sz);                               // coalesce with the free neighbours inside the same chunk
		if (nx != free_.end() && rg && nx->first < rg->first + rg->second) { sz += nx->second; free_.erase(nx); }
		auto pv = free_.lower_bound(p);
		if (pv != free_.begin()) { --pv; if (pv->first + pv->second == p && rg && pv->first >= rg->first) { p = pv->first; sz += pv->second; free_.erase(pv); } }
		free_[p] = sz;
		return true;
	}

	// Takes out the chunks that are one free block each: their bases are appended to `bases`, their bytes returned.
	size_t take_unused_chunks(std::vector<uintptr_t> &bases)
	{
		size_t bytes = 0;
		for (size_t i = 0; i < regions.size(); ) {
			auto it = free_.find(regions[i].first);
			if (it != free_.end() && it->second == regions[i].second) { bases.push_back(regions[i].first); bytes += regions[i].second; free_.erase(it); regions.erase(regions.begin() + (long)i); }
			else ++i;
		}
		return bytes;
	}

	size_t free_bytes() const { size_t f = 0; for (const auto &kv : free_) f += kv.second; return f; }
	void reset_peak() { peak = in_use; }
	const std::map<uintptr_t, size_t> &free_blocks() const { return free_; }

	// The invariants; nullptr when all hold, else the first one that does not.
	const char *check() const
	{
		auto a = free_.begin(); auto b = used_.begin();
		uintptr_t end = 0; bool prev_free = false; const std::pair<uintptr_t, size_t> *prev_rg = nullptr;
		size_t n_free = 0, n_used = 0, n_chunks = 0;
		while (a != free_.end() || b != used_.end()) {                // both maps merged by address
			const bool is_free = b == used_.end() || (a != free_.end() && a->first <= b->first);
			if (is_free && b != used_.end() && a->first == b->first) return "a free and a used block share an address";
			const uintptr_t p = is_free ? a->first : b->first; const size_t sz = is_free ? a->second : b->second;
			if (sz == 0 || sz % ALIGN || p % ALIGN) return "a block is empty or not page-aligned";
			const auto *rg = region_of(p);
			if (!rg || p + sz > rg->first + rg->second) return "a block does not lie inside one chunk";
			if (p < end) return "two blocks overlap";
			if (is_free && prev_free && p == end && rg == prev_rg) return "two free blocks are adjacent within a chunk";
			end = p + sz; prev_free = is_free; prev_rg = rg;
			if (is_free) { n_free += sz; ++a; } else { n_used += sz; ++b; }
		}
		for (const auto &r : regions) n_chunks += r.second;
		if (n_free + n_used != n_chunks) return "used plus free bytes differ from the sum of the chunks";
		if (n_used != in_use) return "in_use differs from the sum of the used blocks";
		if (peak < in_use) return "peak below in_use";
		return nullptr;
	}

private:
	std::map<uintptr_t, size_t> free_;                            // free blocks by address
	std::map<uintptr_t, size_t> used_;                            // handed-out blocks
	const std::pair<uintptr_t, size_t> *region_of(uintptr_t p) const { for (const auto &r : regions) if (p >= r.first && p < r.first + r.second) return &r; return nullptr; }
};

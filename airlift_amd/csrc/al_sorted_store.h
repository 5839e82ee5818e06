// al_sorted_store.h -- the record store of --sorted-bam, shared by the host driver (al_pipeline.cpp) and the stream driver (al_stream_pipe.cpp)
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <unistd.h>
#include <algorithm>
#include <string>
#include <vector>
#include "al_bam.h"
#include "al_env.h"

struct SortedStore {            // --sorted-bam: mapped records are kept until the end of the input, in bounded runs
	std::vector<std::vector<char>> bufs;                  // record bytes, one buffer per (batch, worker)
	std::vector<uint64_t> keys; std::vector<uint32_t> buf_id, off, len;
	size_t bytes = 0, limit = 0;                          // bytes held / spill threshold (samtools sort -m analogue; AL_SORT_MEM, --sort-mem)
	std::vector<FILE *> runs;                             // spilled runs: sorted sequences of (key u64, len u32, record bytes) in unlinked temp files
	al_ctx_t *ctx = nullptr;                              // device that sorts the keys of a run
	size_t held() const { return bytes + keys.size() * 20; }
	// sort what is held (stable radix sort of the keys on the GPU) and stream it to `emit(key, ptr, len)`
	template <class F> int drain_sorted(F emit)
	{
		const size_t n = keys.size();
		std::vector<uint32_t> perm(n);
		if (n && al_sort_keys(ctx, keys.data(), perm.data(), n)) {
			// the device had no room for the keys (the mappers are at their peak when a run is spilled): the same stable order on the host
			fprintf(stderr, "[airlift] --sorted-bam: sorting the keys of this run on the host\n");
			for (size_t i = 0; i < n; ++i) perm[i] = (uint32_t)i;
			std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return keys[x] < keys[y]; });
		}
		for (size_t i = 0; i < n; ++i) { const uint32_t k = perm[i]; if (emit(keys[k], bufs[buf_id[k]].data() + off[k], len[k])) return -3; }
		bufs.clear(); keys.clear(); buf_id.clear(); off.clear(); len.clear(); bytes = 0;
		bufs.shrink_to_fit(); keys.shrink_to_fit(); buf_id.shrink_to_fit(); off.shrink_to_fit(); len.shrink_to_fit();
		return 0;
	}
	int spill()
	{   // one sorted run to a temp file (like samtools sort's -m chunks); merged at the end
		std::string path = std::string(al_env_tmpdir()) + "/airlift_sort_XXXXXX";
		const int fd = mkstemp(&path[0]);
		if (fd < 0) { perror("[airlift] --sorted-bam: cannot create a temporary run file"); return -3; }
		unlink(path.c_str());
		FILE *f = fdopen(fd, "w+b");
		if (!f) { close(fd); return -3; }
		setvbuf(f, nullptr, _IOFBF, 8 << 20);
		const int rc = drain_sorted([&](uint64_t key, const char *p, uint32_t l) { return fwrite(&key, 8, 1, f) != 1 || fwrite(&l, 4, 1, f) != 1 || fwrite(p, 1, l, f) != l; });
		if (rc || fflush(f) == EOF) { fclose(f); fprintf(stderr, "[airlift] --sorted-bam: writing a run file failed\n"); return -3; }
		rewind(f); runs.push_back(f);
		return 0;
	}
	// everything in coordinate order to `emit`: the held records alone, or a k-way merge of the runs (equal keys: earlier run first = input order)
	template <class F> int finish(F emit)
	{
		if (runs.empty()) return drain_sorted([&](uint64_t, const char *p, uint32_t l) { return emit(p, l); });
		if (!keys.empty() && spill()) return -3;
		struct Head { uint64_t key; uint32_t len; size_t run; };
		auto later = [](const Head &a, const Head &b) { return a.key != b.key ? a.key > b.key : a.run > b.run; };
		std::vector<Head> heap; std::vector<char> rec;
		auto next = [&](size_t r) { Head h; h.run = r; if (fread(&h.key, 8, 1, runs[r]) == 1 && fread(&h.len, 4, 1, runs[r]) == 1) { heap.push_back(h); std::push_heap(heap.begin(), heap.end(), later); } };
		for (size_t r = 0; r < runs.size(); ++r) next(r);
		int rc = 0;
		while (!heap.empty() && rc == 0) {
			std::pop_heap(heap.begin(), heap.end(), later); const Head h = heap.back(); heap.pop_back();
			rec.resize(h.len);
			if (h.len && fread(rec.data(), 1, h.len, runs[h.run]) != h.len) { rc = -3; break; }
			if (emit(rec.data(), h.len)) rc = -3;
			next(h.run);
		}
		for (FILE *f : runs) fclose(f);
		runs.clear();
		return rc;
	}
	~SortedStore() { for (FILE *f : runs) fclose(f); }
};

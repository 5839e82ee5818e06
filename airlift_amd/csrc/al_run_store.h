// al_run_store.h -- the store of `lift --sorted`: runs of records that arrive already sorted, merged into one sorted stream.  Host code only, no HIP include;
// tests/csrc/lift_sort_main.cpp runs it under the sanitizers.
//
// SortedStore (al_sorted_store.h) holds an unsorted heap of records and sorts it when it spills.  Here every piece of the lift arrives in key order (the order
// made on the device, or by the twin), so the store only merges.  add_run() copies one piece: its packed record bytes, and per record the key and the length.  A
// run whose first key is not below the last key of the run before it is chained onto that run: a lifted coordinate-sorted BAM is one long chain then, and the
// merge has one source.  When the bytes held pass `limit` (AL_SORT_MEM, --sort-mem; 0: never), ALL held runs are merged k-way into ONE unlinked temp file in
// al_env_tmpdir(), in SortedStore's run format (key u64, len u32, bytes): a whole-genome BAM yields size / limit files, not one per piece.  finish() merges the
// files and the held runs.  Equal keys leave in arrival order: an older file before a newer one, a file before a held run, an earlier run before a later one.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include <unistd.h>
#include <algorithm>
#include <chrono>
#include <string>
#include <vector>
#include "al_env.h"

struct AlRunStore {
	struct Run { std::vector<uint8_t> bytes; std::vector<uint64_t> keys; std::vector<uint32_t> lens; };
	std::vector<Run> held; std::vector<FILE *> files;
	size_t bytes = 0, limit = 0;                               // bytes held (records, keys and lengths) / spill threshold
	uint64_t spills = 0, runs_in = 0, chained = 0, records = 0;
	double emit_s = 0;                                         // seconds inside finish()'s emit
	~AlRunStore() { for (FILE *f : files) fclose(f); }

	// one piece: n records of lens[i] bytes one behind the other at b, keys[] non-decreasing.  0; -3 when a spill fails (its message printed)
	int add_run(const uint8_t *b, size_t nb, const uint64_t *keys, const uint32_t *lens, size_t n)
	{
		if (n == 0) return 0;
		++runs_in; records += n;
		if (!held.empty() && held.back().keys.back() <= keys[0] && held.back().bytes.size() < ((size_t)64 << 20)) ++chained;   // (a chain stays below 64 MB + a piece: no huge vector regrows)
		else held.emplace_back();
		Run &r = held.back();
		r.bytes.insert(r.bytes.end(), b, b + nb); r.keys.insert(r.keys.end(), keys, keys + n); r.lens.insert(r.lens.end(), lens, lens + n);
		bytes += nb + 12 * n;
		return limit && bytes > limit ? spill() : 0;
	}
	// the held runs merged into one temp file
	int spill()
	{
		if (held.empty()) return 0;
		std::string path = std::string(al_env_tmpdir()) + "/airlift_lift_XXXXXX";
		const int fd = mkstemp(&path[0]);
		if (fd < 0) { perror("[airlift] lift --sorted: cannot create a temporary run file"); return -3; }
		unlink(path.c_str());
		FILE *f = fdopen(fd, "w+b");
		if (!f) { close(fd); return -3; }
		setvbuf(f, nullptr, _IOFBF, 1 << 20);
		std::vector<FILE *> none;
		const int rc = merge(none, [&](uint64_t key, const uint8_t *p, uint32_t l) { return fwrite(&key, 8, 1, f) != 1 || fwrite(&l, 4, 1, f) != 1 || (l && fwrite(p, 1, l, f) != l); });
		if (rc || fflush(f) == EOF) { fclose(f); fprintf(stderr, "[airlift] lift --sorted: writing a run file failed\n"); return -3; }
		rewind(f); files.push_back(f); ++spills;
		return 0;
	}
	// everything in key order to emit(bytes, n) -- whole records: a few MB a call from a merge, a run that is the whole output at once; non-zero from emit ends it.  0 or -3
	template <class F> int finish(F emit)
	{
		typedef std::chrono::steady_clock clk;
		int rc = 0;
		auto out = [&](const uint8_t *p, size_t n) { const auto t0 = clk::now(); if (n && emit(p, n)) rc = -3; emit_s += std::chrono::duration<double>(clk::now() - t0).count(); return rc; };
		if (files.empty() && held.size() <= 1) {                       // one chain in memory: it is the output
			if (!held.empty()) out(held[0].bytes.data(), held[0].bytes.size());
			held.clear(); bytes = 0;
			return rc;
		}
		std::vector<uint8_t> buf; buf.reserve(((size_t)4 << 20) + 65536);
		const int mr = merge(files, [&](uint64_t, const uint8_t *p, uint32_t l) {
			if (buf.size() + l > ((size_t)4 << 20) && !buf.empty()) { out(buf.data(), buf.size()); buf.clear(); }
			buf.insert(buf.end(), p, p + l);
			return rc != 0; });
		if (mr == 0 && rc == 0) out(buf.data(), buf.size());
		for (FILE *f : files) fclose(f);
		files.clear();
		return mr ? -3 : rc;
	}

private:
	// The k-way merge of the files `fs` (in order) and the held runs (in order) to sink(key, bytes, len); the held runs are gone afterwards.  A source that has
	// just given a record gives the next ones too while they still come before the head of every other source, so that long stretches cost no heap operation.
	template <class Sink> int merge(std::vector<FILE *> &fs, Sink sink)
	{
		struct Head { uint64_t key; size_t src; };
		auto later = [](const Head &a, const Head &b) { return a.key != b.key ? a.key > b.key : a.src > b.src; };
		const size_t nf = fs.size(), ns = nf + held.size();
		std::vector<size_t> idx(held.size(), 0), off(held.size(), 0); std::vector<uint32_t> flen(nf, 0); std::vector<uint8_t> rec;
		std::vector<Head> heap;
		int rc = 0;
		// the key of source s's next record (files: the 12 bytes in front of the record are read here); false: the source has ended
		auto peek = [&](size_t s, uint64_t *key) {
			if (s < nf) { return fread(key, 8, 1, fs[s]) == 1 && fread(&flen[s], 4, 1, fs[s]) == 1; }
			const Run &r = held[s - nf]; if (idx[s - nf] >= r.keys.size()) return false;
			*key = r.keys[idx[s - nf]]; return true;
		};
		auto take = [&](size_t s, uint64_t key) {
			if (s < nf) {
				rec.resize(flen[s]);
				if (flen[s] && fread(rec.data(), 1, flen[s], fs[s]) != flen[s]) return -3;
				return sink(key, rec.data(), flen[s]) ? -3 : 0;
			}
			const Run &r = held[s - nf]; const size_t i = idx[s - nf]++, o = off[s - nf]; off[s - nf] += r.lens[i];
			return sink(key, r.bytes.data() + o, r.lens[i]) ? -3 : 0;
		};
		for (size_t s = 0; s < ns; ++s) { uint64_t k; if (peek(s, &k)) { heap.push_back(Head{k, s}); std::push_heap(heap.begin(), heap.end(), later); } }
		while (!heap.empty() && rc == 0) {
			std::pop_heap(heap.begin(), heap.end(), later); Head h = heap.back(); heap.pop_back();
			for (;;) {
				if ((rc = take(h.src, h.key)) != 0) break;
				uint64_t k;
				if (!peek(h.src, &k)) break;
				h.key = k;
				if (!heap.empty() && later(h, heap.front())) { heap.push_back(h); std::push_heap(heap.begin(), heap.end(), later); break; }
			}
		}
		held.clear(); held.shrink_to_fit(); bytes = 0;
		return rc;
	}
};

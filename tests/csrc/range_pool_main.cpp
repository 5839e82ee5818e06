// The free list of the device memory reserve (airlift_amd/csrc/al_range_pool.h) on made-up chunks: directed cases of its rules, then a random
// sequence of operations against a page-owner model.  A stand-alone program of host code only -- nothing is allocated behind the addresses
// (tests/test_range_pool_san_cpu.py builds it with AddressSanitizer + UBSan and reads the two counts it prints).  check() runs after every
// operation; the first violation ends the program with a message and a non-zero status.
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <random>
#include "al_range_pool.h"

static const size_t PG = AlRangePool::ALIGN;
static const uintptr_t BASE = (uintptr_t)1 << 32;

#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "range_pool_main.cpp:%d: %s does not hold\n", __LINE__, #cond); exit(1); } } while (0)
static void checked(const AlRangePool &P, const char *after)
{
	if (const char *what = P.check()) { fprintf(stderr, "range_pool_main.cpp: after %s: %s\n", after, what); exit(1); }
}
static uintptr_t A(AlRangePool &P, size_t bytes) { const uintptr_t p = P.alloc(bytes); checked(P, "alloc"); return p; }
static bool F(AlRangePool &P, uintptr_t p) { const bool r = P.free(p); checked(P, "free"); return r; }
static void add(AlRangePool &P, uintptr_t base, size_t pages) { P.add_chunk(base, pages * PG); checked(P, "add_chunk"); }
static size_t take(AlRangePool &P, std::vector<uintptr_t> &bases) { bases.clear(); const size_t b = P.take_unused_chunks(bases); checked(P, "take_unused_chunks"); return b; }

static void directed()
{
	std::vector<uintptr_t> bases;
	{   // an empty pool
		AlRangePool P; checked(P, "construction");
		REQUIRE(A(P, 1) == 0); REQUIRE(!F(P, BASE)); REQUIRE(P.free_bytes() == 0); REQUIRE(take(P, bases) == 0 && bases.empty());
		REQUIRE(P.n_served == 0 && P.in_use == 0 && P.peak == 0);
	}
	{   // one chunk of 16 pages: requests are rounded up to pages and served from the base upwards
		AlRangePool P; add(P, BASE, 16);
		REQUIRE(A(P, 1) == BASE); REQUIRE(P.in_use == PG);
		REQUIRE(A(P, 4097) == BASE + PG); REQUIRE(P.in_use == 3 * PG);
		REQUIRE(A(P, 1) == BASE + 3 * PG);
	}
	{   // the whole chunk is served, a page more is not
		AlRangePool P; add(P, BASE, 16);
		REQUIRE(A(P, 16 * PG + 1) == 0); REQUIRE(A(P, 17 * PG) == 0); REQUIRE(P.n_served == 0);
		REQUIRE(A(P, 16 * PG) == BASE); REQUIRE(P.free_bytes() == 0); REQUIRE(A(P, 1) == 0);
	}
	{   // holes of 3, 1 and 2 pages with used pages between them: two pages go into the hole of two
		AlRangePool P; add(P, BASE, 16);
		REQUIRE(A(P, 3 * PG) == BASE); REQUIRE(A(P, PG) == BASE + 3 * PG); REQUIRE(A(P, PG) == BASE + 4 * PG); REQUIRE(A(P, PG) == BASE + 5 * PG);
		REQUIRE(A(P, 2 * PG) == BASE + 6 * PG); REQUIRE(A(P, PG) == BASE + 8 * PG); REQUIRE(A(P, 7 * PG) == BASE + 9 * PG);
		REQUIRE(F(P, BASE)); REQUIRE(F(P, BASE + 4 * PG)); REQUIRE(F(P, BASE + 6 * PG));
		REQUIRE(P.free_blocks().size() == 3 && P.free_bytes() == 6 * PG);
		REQUIRE(A(P, 2 * PG - 5) == BASE + 6 * PG);
		REQUIRE(A(P, 1) == BASE + 4 * PG);                             // (and one page into the hole of one)
		REQUIRE(A(P, 2 * PG) == BASE);                                 // (what is left: the hole of three, split)
		REQUIRE(P.free_blocks().size() == 1 && P.free_blocks().begin()->first == BASE + 2 * PG && P.free_bytes() == PG);
	}
	{   // holes of 3, 2 and 2 pages: of the two that fit best, the lower one
		AlRangePool P; add(P, BASE, 16);
		REQUIRE(A(P, 3 * PG) == BASE); REQUIRE(A(P, PG) == BASE + 3 * PG); REQUIRE(A(P, 2 * PG) == BASE + 4 * PG); REQUIRE(A(P, PG) == BASE + 6 * PG);
		REQUIRE(A(P, 2 * PG) == BASE + 7 * PG); REQUIRE(A(P, 7 * PG) == BASE + 9 * PG);
		REQUIRE(F(P, BASE + 7 * PG)); REQUIRE(F(P, BASE)); REQUIRE(F(P, BASE + 4 * PG));
		REQUIRE(A(P, PG + 1) == BASE + 4 * PG);
		REQUIRE(A(P, PG + 1) == BASE + 7 * PG);
	}
	{   // three neighbouring ranges that fill a chunk, freed in each of the six orders: one block in the end, and the chunk can go
		int order[3] = {0, 1, 2}; int n_orders = 0;
		do {
			AlRangePool P; add(P, BASE, 16);
			const uintptr_t at[3] = {A(P, 5 * PG), A(P, 3 * PG), A(P, 8 * PG)};
			REQUIRE(at[0] == BASE && at[1] == BASE + 5 * PG && at[2] == BASE + 8 * PG); REQUIRE(P.free_bytes() == 0);
			REQUIRE(take(P, bases) == 0);                                 // (in use: it stays)
			REQUIRE(F(P, at[order[0]])); REQUIRE(P.free_blocks().size() == 1);
			REQUIRE(F(P, at[order[1]])); REQUIRE(P.free_blocks().size() == (order[0] + order[1] == 2 ? 2u : 1u));   // (the outer two do not touch)
			REQUIRE(take(P, bases) == 0 && P.regions.size() == 1);
			REQUIRE(F(P, at[order[2]]));
			REQUIRE(P.free_blocks().size() == 1 && P.free_blocks().begin()->first == BASE && P.free_blocks().begin()->second == 16 * PG && P.in_use == 0);
			REQUIRE(take(P, bases) == 16 * PG && bases.size() == 1 && bases[0] == BASE);
			REQUIRE(P.regions.empty() && P.free_bytes() == 0 && A(P, 1) == 0);
			++n_orders;
		} while (std::next_permutation(order, order + 3));
		REQUIRE(n_orders == 6);
	}
	for (int b_first = 0; b_first < 2; ++b_first) {   // two chunks, the second beginning where the first ends: free blocks on either side of the seam stay apart, whichever is freed first
		AlRangePool P; add(P, BASE, 8); add(P, BASE + 8 * PG, 8);
		const uintptr_t a = A(P, 5 * PG), b = A(P, 3 * PG), c = A(P, 3 * PG), d = A(P, 5 * PG);
		REQUIRE(a == BASE && b == BASE + 5 * PG && c == BASE + 8 * PG && d == BASE + 11 * PG);
		REQUIRE(F(P, b_first ? b : c)); REQUIRE(F(P, b_first ? c : b));
		REQUIRE(P.free_blocks().size() == 2 && P.free_bytes() == 6 * PG);
		REQUIRE(P.free_blocks().begin()->first == b && P.free_blocks().begin()->second == 3 * PG && P.free_blocks().rbegin()->first == c && P.free_blocks().rbegin()->second == 3 * PG);
		REQUIRE(A(P, 3 * PG + 1) == 0); REQUIRE(A(P, 6 * PG) == 0);
		// the first chunk entirely free, the second holding one range: only the first is taken out
		REQUIRE(F(P, a)); REQUIRE(P.free_blocks().size() == 2 && P.free_blocks().begin()->second == 8 * PG);
		REQUIRE(take(P, bases) == 8 * PG && bases.size() == 1 && bases[0] == BASE);
		REQUIRE(P.regions.size() == 1 && P.regions[0].first == BASE + 8 * PG && P.free_bytes() == 3 * PG && P.in_use == 5 * PG);
		REQUIRE(!F(P, a)); REQUIRE(!F(P, b));                          // what the removed chunk once handed out is nobody's now
		REQUIRE(A(P, 4 * PG) == 0);                                    // (8 pages were free there)
		REQUIRE(A(P, 3 * PG) == c);
		REQUIRE(F(P, d)); REQUIRE(F(P, c));
		REQUIRE(P.free_blocks().size() == 1 && P.free_blocks().begin()->first == BASE + 8 * PG);
		REQUIRE(take(P, bases) == 8 * PG && bases[0] == BASE + 8 * PG && P.regions.empty());
	}
	{   // only the start of a handed-out range frees it, and only once
		AlRangePool P; add(P, BASE, 16);
		const uintptr_t a = A(P, 2 * PG);
		REQUIRE(!F(P, a + PG)); REQUIRE(!F(P, a + 1)); REQUIRE(!F(P, a + 2 * PG)); REQUIRE(!F(P, BASE - PG)); REQUIRE(!F(P, 0));
		REQUIRE(P.in_use == 2 * PG);
		REQUIRE(F(P, a)); REQUIRE(!F(P, a)); REQUIRE(P.in_use == 0);
	}
	{   // the counters, step by step
		AlRangePool P; add(P, BASE, 16);
		REQUIRE(P.free_bytes() == 16 * PG && P.in_use == 0 && P.peak == 0 && P.n_served == 0);
		const uintptr_t a = A(P, 1);            REQUIRE(P.in_use == 1 * PG && P.peak == 1 * PG && P.free_bytes() == 15 * PG && P.n_served == 1);
		const uintptr_t b = A(P, 3 * PG + 1);   REQUIRE(P.in_use == 5 * PG && P.peak == 5 * PG && P.free_bytes() == 11 * PG && P.n_served == 2);
		REQUIRE(F(P, a));                       REQUIRE(P.in_use == 4 * PG && P.peak == 5 * PG && P.free_bytes() == 12 * PG && P.n_served == 2);
		P.reset_peak(); checked(P, "reset_peak"); REQUIRE(P.in_use == 4 * PG && P.peak == 4 * PG);
		REQUIRE(A(P, 2 * PG) == BASE + 5 * PG); REQUIRE(P.in_use == 6 * PG && P.peak == 6 * PG && P.free_bytes() == 10 * PG && P.n_served == 3);
		REQUIRE(A(P, 10 * PG) == 0);            REQUIRE(P.in_use == 6 * PG && P.peak == 6 * PG && P.free_bytes() == 10 * PG && P.n_served == 3);   // (9 + 1 pages free, apart)
		REQUIRE(!F(P, b + PG));                 REQUIRE(P.in_use == 6 * PG && P.free_bytes() == 10 * PG);
		REQUIRE(F(P, b));                       REQUIRE(P.in_use == 2 * PG && P.peak == 6 * PG && P.free_bytes() == 14 * PG);
		P.reset_peak();                         REQUIRE(P.peak == 2 * PG);
	}
	{   // a request of no bytes is not served, and leaves the address to the next request
		AlRangePool P; add(P, BASE, 16);
		REQUIRE(A(P, 0) == 0); REQUIRE(P.n_served == 0 && P.in_use == 0 && P.free_blocks().size() == 1);
		REQUIRE(A(P, 1) == BASE);
		REQUIRE(A(P, 0) == 0); REQUIRE(P.n_served == 1 && P.in_use == PG);
		REQUIRE(A(P, 1) == BASE + PG);
	}
}

// ---- random operations against a model: who owns each page of each chunk ----
struct Chunk { uintptr_t base; size_t pages; bool present; std::vector<int> owner; };   // owner: 0 = free, else the range's id
struct Live { int id; uintptr_t at; size_t pages; };

static void randomised()
{
	Chunk ch[3] = {{BASE, 64, true, {}}, {BASE + 64 * PG, 64, true, {}}, {BASE + 1024 * PG, 32, true, {}}};   // the first two are address-adjacent
	AlRangePool P;
	for (Chunk &c : ch) { c.owner.assign(c.pages, 0); add(P, c.base, c.pages); }
	std::vector<Live> live; std::vector<uintptr_t> bases;
	std::mt19937_64 rng(20250917);
	size_t n_served = 0, n_refused = 0, in_use = 0; int next_id = 1;
	for (int op = 0; op < 20000; ++op) {
		const unsigned r = (unsigned)(rng() % 100);
		if (r < 50 || (r < 88 && live.empty())) {                     // allocate 1 ... 20 pages' worth of bytes, never a multiple of the page
			const size_t np = 1 + (size_t)(rng() % 20), bytes = (np - 1) * PG + 1 + (size_t)(rng() % (PG - 1));
			// the model's answer: the start of the smallest free run of at least np pages, the lowest address among equals; runs end at chunk ends
			uintptr_t want = 0; size_t want_len = 0;
			for (const Chunk &c : ch) {
				if (!c.present) continue;
				for (size_t i = 0; i < c.pages; ) {
					if (c.owner[i]) { ++i; continue; }
					size_t j = i; while (j < c.pages && !c.owner[j]) ++j;
					if (j - i >= np && (!want || j - i < want_len)) { want = c.base + i * PG; want_len = j - i; }
					i = j;
				}
			}
			const uintptr_t got = A(P, bytes);
			if (got != want) { fprintf(stderr, "range_pool_main.cpp: operation %d: %zu pages served at %#zx, the model says %#zx\n", op, np, (size_t)got, (size_t)want); exit(1); }
			if (!got) ++n_refused;
			else {
				REQUIRE(got % PG == 0);
				Chunk *in = nullptr; for (Chunk &c : ch) if (c.present && got >= c.base && got + np * PG <= c.base + c.pages * PG) in = &c;
				REQUIRE(in != nullptr);                                    // inside one chunk
				for (size_t i = 0; i < np; ++i) { int &o = in->owner[(got - in->base) / PG + i]; REQUIRE(o == 0); o = next_id; }   // overlaps no live range
				live.push_back(Live{next_id++, got, np}); ++n_served; in_use += np * PG;
			}
		} else if (r < 88) {                                           // free a live range
			const size_t k = (size_t)(rng() % live.size()); const Live v = live[k];
			live[k] = live.back(); live.pop_back();
			REQUIRE(F(P, v.at));
			for (Chunk &c : ch) if (v.at >= c.base && v.at < c.base + c.pages * PG) for (size_t i = 0; i < v.pages; ++i) { REQUIRE(c.owner[(v.at - c.base) / PG + i] == v.id); c.owner[(v.at - c.base) / PG + i] = 0; }
			in_use -= v.pages * PG;
		} else if (r < 96) {                                           // free an address picked blindly: a page of some chunk (present or not), or just off a page, or outside every chunk
			const Chunk &c = ch[rng() % 3];
			uintptr_t at = c.base + (uintptr_t)(rng() % (c.pages + 2)) * PG - PG;
			if (rng() % 4 == 0) at += 1 + (uintptr_t)(rng() % (PG - 1));
			size_t k = 0; while (k < live.size() && live[k].at != at) ++k;
			if (k < live.size()) { --op; continue; }                     // (that one is somebody's: not this branch's business)
			REQUIRE(!F(P, at));
		} else if (r < 98) {                                           // take out the chunks nothing is using
			size_t want_bytes = 0; std::vector<uintptr_t> want;
			for (Chunk &c : ch) if (c.present && std::all_of(c.owner.begin(), c.owner.end(), [](int o) { return o == 0; })) { want.push_back(c.base); want_bytes += c.pages * PG; c.present = false; }
			REQUIRE(take(P, bases) == want_bytes);
			std::sort(bases.begin(), bases.end()); REQUIRE(bases == want);
		} else {                                                       // and add them back
			for (Chunk &c : ch) if (!c.present) { add(P, c.base, c.pages); c.present = true; }
		}
		REQUIRE(P.in_use == in_use && P.n_served == n_served && P.peak >= in_use);
		size_t free_pages = 0; for (const Chunk &c : ch) if (c.present) free_pages += (size_t)std::count(c.owner.begin(), c.owner.end(), 0);
		REQUIRE(P.free_bytes() == free_pages * PG);
	}
	printf("random served %zu refused %zu\n", n_served, n_refused);
}

int main()
{
	directed();
	printf("directed ok\n");
	randomised();
	return 0;
}

// merge_main.cpp -- the merge of `airlift-align merge` on the host, stand-alone under AddressSanitizer + UBSan (`make san-merge`): the headers' merge, the kernels'
// twin (al_dev_merge.h), the window rule and the round loop (al_merge.h), host code only.
//
//   san_merge [TILE]     TILE: the tile the ties shapes are sized by (default AL_MERGE_TILE)
//
// The shapes are generated here from the tables tests/merge_cases.py holds as san_specs(): the windows shapes at pieces of 1000 and 4096 bytes, the ties shapes,
// the unsorted shapes.  Every shape goes through the twin's round loop with each stream whole (one round), at pieces of 1000, 4096 and 65536 bytes and, for a
// shape of at most 32 KB, at every piece size from 64 bytes to 256 and then at sizes growing by 1/16: a descent then falls on a window's end at some size.  Each
// stream lies in a heap buffer of exactly its size.  The merged bytes must be the same at every size.  One line per shape -- records, rounds at 1000 bytes and
// the FNV-1a digest of the merged records, or the code of a refusal and its offset -- then "san_merge: N shapes".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "al_merge.h"

struct Seg { int rid, pos0, step, count; std::string pre; };
typedef std::vector<std::vector<Seg>> Spec;
struct Shape { std::string name; Spec spec; };

static const char *HEADER = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chrA\tLN:10000\n@SQ\tSN:chrB\tLN:8000\n@SQ\tSN:chrC\tLN:5000\n@PG\tID:x\tPN:x\n";
static const struct { const char *name; uint32_t len; } REFS[3] = {{"chrA", 10000}, {"chrB", 8000}, {"chrC", 5000}};

static void p32(std::vector<uint8_t> &o, uint32_t v) { for (int i = 0; i < 4; ++i) o.push_back((uint8_t)(v >> (8 * i))); }
static void p16(std::vector<uint8_t> &o, uint32_t v) { o.push_back((uint8_t)v); o.push_back((uint8_t)(v >> 8)); }
// the record lift_cases.rec_bytes makes of merge_cases.R (10M, MAPQ 30, no mate, no sequence) or, rid < 0, of merge_cases.U (unmapped, no CIGAR)
static void put_rec(std::vector<uint8_t> &o, int rid, int pos, const std::string &name)
{
	const bool un = rid < 0;
	p32(o, 32 + (uint32_t)name.size() + 1 + (un ? 0 : 4));
	p32(o, (uint32_t)rid); p32(o, (uint32_t)pos); o.push_back((uint8_t)(name.size() + 1)); o.push_back(30); p16(o, 4680); p16(o, un ? 0 : 1); p16(o, un ? 4 : 0);
	p32(o, 0); p32(o, 0xffffffffu); p32(o, 0xffffffffu); p32(o, 0);
	o.insert(o.end(), name.begin(), name.end()); o.push_back(0);
	if (!un) p32(o, 10u << 4);
}
static std::vector<uint8_t> stream_of(const std::vector<Seg> &segs)
{
	std::vector<uint8_t> o = {'B', 'A', 'M', 1};
	p32(o, (uint32_t)strlen(HEADER)); o.insert(o.end(), HEADER, HEADER + strlen(HEADER)); p32(o, 3);
	for (const auto &r : REFS) { p32(o, (uint32_t)strlen(r.name) + 1); o.insert(o.end(), r.name, r.name + strlen(r.name) + 1); p32(o, r.len); }
	for (const Seg &s : segs) for (int i = 0; i < s.count; ++i) put_rec(o, s.rid, s.rid < 0 ? -1 : s.pos0 + i * s.step, s.pre + std::to_string(i));
	return o;
}
static std::vector<Shape> shapes(int T)
{
	std::vector<Shape> out;
	for (int p : {1000, 4096}) {
		const int n = p / 45 + 1; const std::string w = "w" + std::to_string(p) + "_";
		Spec ca = {{{0, 100, 1, n / 2, "al"}, {0, 5000, 0, n, "ae"}, {0, 6000, 1, n, "ah"}}, {{0, 50, 1, 3, "bl"}, {0, 5000, 0, 3, "be"}, {0, 5500, 1, 2 * n, "bh"}}};
		out.push_back({w + "cross_a", ca});
		out.push_back({w + "cross_b", {ca[1], ca[0]}});
		out.push_back({w + "dense", {{{0, 10, 1, 8 * n, "a"}}, {{0, 10, 2 * n, 5, "b"}}}});
		out.push_back({w + "header_only", {{{0, 100, 1, 2 * n, "al"}}, {}}});
		for (int k : {3, 8}) {
			Spec s;
			for (int i = 0; i < k; ++i) { const std::string c(1, (char)('a' + i)); s.push_back({{0, 100 + i, 1, n / 2 + i, c + "l"}, {0, 5000, 0, n / 3 + 2 * i + 1, c + "e"}, {0, 6000 + i, 1, n / 2, c + "h"}}); }
			out.push_back({w + "k" + std::to_string(k), s});
		}
		out.push_back({w + "early_eof", {{{0, 10, 1, 3, "al"}}, {{0, 5, 1, 3 * n, "bl"}}, {{0, 7, 1, 2, "cl"}}}});
	}
	out.push_back({"all_equal", {{{0, 100, 0, T + 1, "a"}}, {{0, 100, 0, T + 1, "b"}}}});
	out.push_back({"straddle", {{{0, 10, 1, 5, "al"}, {0, 500, 0, 2 * T, "a"}, {0, 900, 1, 1, "ah"}}, {{0, 20, 1, 3, "bl"}, {0, 500, 0, 2 * T, "b"}, {0, 901, 1, 2, "bh"}}}});
	out.push_back({"unmapped_both", {{{0, 10, 3, 20, "a"}, {1, 10, 3, 20, "aa"}, {-1, -1, 0, 3, "au"}}, {{0, 11, 3, 20, "b"}, {1, 11, 3, 20, "bb"}, {-1, -1, 0, 4, "bu"}}}});
	out.push_back({"unsorted_mid", {{{0, 100, 10, 60, "a"}}, {{0, 100, 10, 7, "b"}, {0, 100, 0, 1, "down"}, {0, 180, 10, 40, "c"}}}});
	out.push_back({"unsorted_after_unmapped", {{{0, 100, 10, 60, "a"}}, {{0, 100, 1, 1, "b"}, {-1, -1, 0, 1, "u"}, {0, 200, 1, 1, "after"}}}});
	out.push_back({"unsorted_first", {{{0, 100, 10, 30, "a"}, {0, 90, 1, 1, "down"}}, {{0, 5, 1, 50, "b"}}}});
	return out;
}
static uint64_t fnv(uint64_t h, const void *p, size_t n) { const uint8_t *s = (const uint8_t *)p; for (size_t i = 0; i < n; ++i) { h ^= s[i]; h *= 0x100000001b3ull; } return h; }

int main(int argc, char **argv)
{
	const int T = argc > 1 ? atoi(argv[1]) : (int)AL_MERGE_TILE;
	if (T < 2) { fprintf(stderr, "usage: san_merge [TILE]\n"); return 2; }
	int n_shapes = 0;
	for (const Shape &S : shapes(T)) {
		const int k = (int)S.spec.size();
		std::vector<void *> heap; std::vector<const void *> bam; std::vector<size_t> n; size_t total = 0;
		for (const auto &segs : S.spec) { const std::vector<uint8_t> b = stream_of(segs); void *p = malloc(b.size()); memcpy(p, b.data(), b.size()); heap.push_back(p); bam.push_back(p); n.push_back(b.size()); total += b.size(); }
		std::vector<size_t> pieces = {0, 1000, 4096, 65536};
		if (total <= 32768) { for (size_t p = 64; p <= 256; ++p) pieces.push_back(p); for (size_t p = 272; p < total; p += p / 16) pieces.push_back(p); }
		const size_t rec_cap = total / 36 + 2;
		std::vector<uint32_t> tags(rec_cap); std::vector<uint64_t> keys(rec_cap); std::vector<uint8_t> packed(total + 1);
		int rc0 = 0; uint64_t h0 = 0, rounds1000 = 0; size_t n0 = 0;
		for (size_t q = 0; q < pieces.size(); ++q) {
			AlMergeHostBackend B; size_t n_out = 0, packed_n = 0; uint64_t rounds = 0;
			const int rc = al_merge_tap(B, bam.data(), n.data(), k, pieces[q], tags.data(), keys.data(), rec_cap, &n_out, packed.data(), packed.size(), &packed_n, &rounds);
			if (rc == -1 || rc == -3 || rc == -4) { printf("%s: piece %zu: al_merge_tap returned %d\n", S.name.c_str(), pieces[q], rc); return 1; }
			uint64_t h = fnv(0xcbf29ce484222325ull, packed.data(), rc == 0 ? packed_n : 0);
			for (size_t i = 1; rc == 0 && i < n_out; ++i) if (keys[i] < keys[i - 1]) { printf("%s: piece %zu: the merged keys descend at %zu\n", S.name.c_str(), pieces[q], i); return 1; }
			if (q == 0) { rc0 = rc; h0 = h; n0 = n_out; if (rc == 0 && rounds != 1) { printf("%s: %llu rounds for whole streams\n", S.name.c_str(), (unsigned long long)rounds); return 1; } }
			else if (rc != rc0 || (rc == 0 && (h != h0 || n_out != n0))) { printf("%s: piece %zu differs from the whole streams (%d / %d, %zu / %zu records)\n", S.name.c_str(), pieces[q], rc, rc0, n_out, n0); return 1; }
			if (pieces[q] == 1000) rounds1000 = rounds;
		}
		if (rc0 == 0) printf("%s records=%zu rounds=%llu digest=%016llx\n", S.name.c_str(), n0, (unsigned long long)rounds1000, (unsigned long long)h0);
		else printf("%s refused=%d\n", S.name.c_str(), rc0);
		for (void *p : heap) free(p);
		++n_shapes;
	}
	printf("san_merge: %d shapes\n", n_shapes);
	return 0;
}

// index_main.cpp -- the index of `airlift-align bam-index` on the host, stand-alone under AddressSanitizer + UBSan (`make san-bai`): the kernels' twin
// (al_dev_bai.h), the member table, the piece / carry loop and the file's assembly (al_bai.h), host code only.
//
//   san_bai
//
// The shapes are generated here from the tables tests/index_cases.py holds as san_specs(): runs of one bin, bins of several levels, several contigs with unplaced
// records at the tail, records at the top of a contig of 2^29, a header alone, and the inputs that are refused.  The member table is synthetic: members of 333
// stream bytes, member k at file offset 1000 k.  Every shape goes through the twin's loop with the stream whole, at pieces of 1000, 4096 and 65536 bytes and, for a
// shape of at most 32 KB, at every piece size from 64 bytes to 256 and then at sizes growing by 1/16: a run then ends on a piece's end at some size, and a record on
// a member's.  The stream lies in a heap buffer of exactly its size.  The index must be the same at every size.  One line per shape -- the bytes of the index and
// their FNV-1a digest, or the code of a refusal -- then "san_bai: N shapes".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "al_bai.h"

struct Seg { int rid, pos0, step, count, reflen; std::string pre; };
struct Shape { std::string name; std::vector<Seg> segs; };

static const struct { const char *name; uint32_t len; } REFS[5] = {{"big", 1u << 29}, {"s1", 100000}, {"none_mid", 5000}, {"s2", 70000}, {"none_end", 3000}};
static const size_t MEMBER = 333;

static void p32(std::vector<uint8_t> &o, uint32_t v) { for (int i = 0; i < 4; ++i) o.push_back((uint8_t)(v >> (8 * i))); }
static void p16(std::vector<uint8_t> &o, uint32_t v) { o.push_back((uint8_t)v); o.push_back((uint8_t)(v >> 8)); }
// the record lift_cases.rec_bytes makes of index_cases.M (one M operation, MAPQ 30, no mate, no sequence) or, rid < 0, of index_cases.U (unplaced, no CIGAR)
static void put_rec(std::vector<uint8_t> &o, int rid, int pos, int reflen, const std::string &name)
{
	const bool un = rid < 0;
	p32(o, 32 + (uint32_t)name.size() + 1 + (un ? 0 : 4));
	p32(o, (uint32_t)rid); p32(o, (uint32_t)pos); o.push_back((uint8_t)(name.size() + 1)); o.push_back(30); p16(o, 4680); p16(o, un ? 0 : 1); p16(o, un ? 4 : 0);
	p32(o, 0); p32(o, 0xffffffffu); p32(o, 0xffffffffu); p32(o, 0);
	o.insert(o.end(), name.begin(), name.end()); o.push_back(0);
	if (!un) p32(o, (uint32_t)reflen << 4);
}
static std::vector<uint8_t> stream_of(const std::vector<Seg> &segs)
{
	std::string text = "@HD\tVN:1.6\tSO:coordinate\n";
	for (const auto &r : REFS) text += std::string("@SQ\tSN:") + r.name + "\tLN:" + std::to_string(r.len) + "\n";
	std::vector<uint8_t> o = {'B', 'A', 'M', 1};
	p32(o, (uint32_t)text.size()); o.insert(o.end(), text.begin(), text.end()); p32(o, 5);
	for (const auto &r : REFS) { p32(o, (uint32_t)strlen(r.name) + 1); o.insert(o.end(), r.name, r.name + strlen(r.name) + 1); p32(o, r.len); }
	for (const Seg &s : segs) for (int i = 0; i < s.count; ++i) put_rec(o, s.rid, s.rid < 0 ? -1 : s.pos0 + i * s.step, s.reflen, s.pre + std::to_string(i));
	return o;
}
static std::vector<Shape> shapes()
{
	const int top = (1 << 29);
	return {{"one_bin", {{0, 10, 1, 300, 10, "o"}}},
	        {"bins", {{0, 10, 4000, 40, 20000, "w"}, {0, 200000, 16384, 30, 10, "n"}, {1, 5, 7, 100, 30, "s"}}},
	        {"contigs", {{0, 100, 50, 20, 10, "a"}, {1, 100, 50, 20, 10, "b"}, {3, 100, 50, 20, 10, "c"}, {-1, -1, 0, 5, 0, "u"}}},
	        {"top", {{0, top - 1000, 10, 90, 100, "t"}}},
	        {"header_only", {}},
	        {"refused_descent", {{1, 100, 10, 30, 10, "a"}, {1, 90, 1, 1, 10, "down"}, {1, 500, 10, 30, 10, "b"}}},
	        {"refused_after_unplaced", {{1, 100, 10, 3, 10, "a"}, {-1, -1, 0, 1, 0, "u"}, {1, 900, 1, 1, 10, "z"}}},
	        {"refused_big", {{0, top - 5, 1, 1, 10, "big"}}},
	        {"refused_ln", {{3, 69995, 1, 1, 10, "over"}}}};
}
static uint64_t fnv(const void *p, size_t n) { uint64_t h = 0xcbf29ce484222325ull; const uint8_t *s = (const uint8_t *)p; for (size_t i = 0; i < n; ++i) { h ^= s[i]; h *= 0x100000001b3ull; } return h; }

int main()
{
	int n_shapes = 0;
	for (const Shape &S : shapes()) {
		const std::vector<uint8_t> b = stream_of(S.segs);
		uint8_t *heap = (uint8_t *)malloc(b.size()); memcpy(heap, b.data(), b.size());
		const size_t k = (b.size() + MEMBER - 1) / MEMBER;
		std::vector<uint64_t> m_file(k), m_stream(k); std::vector<uint32_t> m_isize(k);
		for (size_t i = 0; i < k; ++i) { m_file[i] = 1000 * i; m_stream[i] = MEMBER * i; m_isize[i] = (uint32_t)std::min(MEMBER, b.size() - MEMBER * i); }
		std::vector<size_t> pieces = {0, 1000, 4096, 65536};
		if (b.size() <= 32768) { for (size_t p = 64; p <= 256; ++p) pieces.push_back(p); for (size_t p = 272; p < b.size(); p += p / 16) pieces.push_back(p); }
		int rc0 = 0; std::vector<uint8_t> bai0;
		for (size_t q = 0; q < pieces.size(); ++q) {
			AlBaiHostBackend B; std::vector<uint8_t> bai;
			const int rc = al_bai_tap(B, heap, b.size(), m_file.data(), m_stream.data(), m_isize.data(), k, 1000 * k, pieces[q], bai);
			if (rc == -1 || rc == -4) { printf("%s: piece %zu: al_bai_tap returned %d\n", S.name.c_str(), pieces[q], rc); return 1; }
			if (q == 0) { rc0 = rc; bai0 = bai; }
			else if (rc != rc0 || (rc == 0 && bai != bai0)) { printf("%s: piece %zu differs from the whole stream (%d / %d, %zu / %zu bytes)\n", S.name.c_str(), pieces[q], rc, rc0, bai.size(), bai0.size()); return 1; }
		}
		if (rc0 == 0) printf("%s bytes=%zu digest=%016llx\n", S.name.c_str(), bai0.size(), (unsigned long long)fnv(bai0.data(), bai0.size()));
		else printf("%s refused=%d\n", S.name.c_str(), rc0);
		free(heap);
		++n_shapes;
	}
	printf("san_bai: %d shapes\n", n_shapes);
	return 0;
}

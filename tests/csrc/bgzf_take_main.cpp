// bgzf_take_main.cpp -- the listing-and-take function of the stream driver's BGZF input (airlift_amd/csrc/al_bgzf_take.h) as a stand-alone host program
// for AddressSanitizer + UBSan (`make san-bgzf-take`; tests/test_bgzf_take_san_cpu.py).  argv[1]: a file of BGZF members back to back.  The members of a
// single-piece run (the whole file fed at once, one take) are the expectation; then the file is fed in pieces of every size from 1 byte up to twice the
// largest member, through a window of exactly piece + 65536 heap bytes, with takes of changing want / member / byte limits, and every member must come
// out once, in order, with the same offsets.  Prints one line; exit 1 on any difference.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "al_bgzf_take.h"

struct Abs { uint64_t in_off, out_off; uint32_t msize, isize; };

static bool run(const std::vector<uint8_t> &file, size_t piece, uint64_t want0, uint64_t max_in, size_t max_mem, std::vector<Abs> &got, uint64_t *calls)
{
	AlBgzfFeed f; f.cap = piece + 65536; f.buf = (uint8_t *)malloc(f.cap);
	size_t fpos = 0; bool eof = false, ok = true; uint64_t round = 0;
	std::vector<AlInfMember> mem;
	got.clear();
	for (;;) {
		const uint8_t *bytes = nullptr; uint64_t n_in = 0, n_out = 0, at = 0;
		const uint64_t in0 = f.file_off, out0 = f.out_off;
		const uint64_t want = want0 ? 1 + (want0 * (round % 5 + 1)) % 200000 : ~0ull; ++round;
		const int r = al_bgzf_take(f, want, max_in, max_mem, mem, &bytes, &n_in, &n_out, &at);
		++*calls;
		if (at != in0) { fprintf(stderr, "file_off_at %llu, expected %llu\n", (unsigned long long)at, (unsigned long long)in0); ok = false; break; }
		uint64_t si = 0, so = 0;
		for (const AlInfMember &m : mem) {
			if (m.in_off != si || m.out_off != so || memcmp(bytes + m.in_off, file.data() + in0 + m.in_off, m.msize) != 0) { fprintf(stderr, "a member's offsets or bytes are off\n"); ok = false; }
			got.push_back(Abs{in0 + m.in_off, out0 + m.out_off, m.msize, m.isize}); si += m.msize; so += m.isize;
		}
		if (si != n_in || so != n_out || f.file_off != in0 + n_in || f.out_off != out0 + n_out) { fprintf(stderr, "the sums are off\n"); ok = false; }
		if (mem.size() > max_mem || n_in > max_in) { fprintf(stderr, "a limit was passed\n"); ok = false; }
		if (r == AL_BGZF_COVERED && n_out < want) { fprintf(stderr, "covered, but short\n"); ok = false; }
		if (!ok || r == AL_BGZF_BROKEN) { if (r == AL_BGZF_BROKEN) { fprintf(stderr, "chain broken at %llu\n", (unsigned long long)f.file_off); ok = false; } break; }
		if (r == AL_BGZF_MORE) {
			if (eof) { if (al_bgzf_feed_left(f)) { fprintf(stderr, "bytes left at the end\n"); ok = false; } break; }
			size_t room = 0; uint8_t *dst = al_bgzf_feed_room(f, &room);
			if (room < piece) { fprintf(stderr, "no room for a piece behind the carry\n"); ok = false; break; }
			const size_t n = file.size() - fpos < piece ? file.size() - fpos : piece;
			memcpy(dst, file.data() + fpos, n); al_bgzf_feed_add(f, n); fpos += n;
			if (fpos == file.size()) eof = true;
		}
	}
	free(f.buf);
	return ok;
}

int main(int argc, char **argv)
{
	if (argc < 2) { fprintf(stderr, "usage: san_bgzf_take members.bgzf\n"); return 2; }
	FILE *fp = fopen(argv[1], "rb");
	if (!fp) { perror(argv[1]); return 2; }
	std::vector<uint8_t> file; uint8_t tmp[65536]; size_t g;
	while ((g = fread(tmp, 1, sizeof(tmp), fp)) > 0) file.insert(file.end(), tmp, tmp + g);
	fclose(fp);
	std::vector<Abs> ref, got; uint64_t calls = 0;
	if (!run(file, file.size() ? file.size() : 1, 0, ~0ull, (size_t)-1, ref, &calls)) return 1;
	uint32_t largest = 0; uint64_t in_sum = 0;
	for (const Abs &a : ref) { if (a.msize > largest) largest = a.msize; in_sum += a.msize; }
	if (in_sum != file.size() || ref.empty()) { fprintf(stderr, "the single-piece run did not take the whole file\n"); return 1; }
	uint64_t runs = 0;
	for (size_t piece = 1; piece <= 2 * (size_t)largest; ++piece) {
		// limits go round with the piece size: no limit, few members per take, few bytes per take (never less than one member), small wants
		const size_t max_mem = piece % 3 == 0 ? 1 + piece % 7 : (size_t)-1;
		const uint64_t max_in = piece % 3 == 1 ? (uint64_t)largest + piece % 1000 : ~0ull;
		const uint64_t want0 = piece % 2 ? 0 : 1 + piece * 37 % 5000;
		if (!run(file, piece, want0, max_in, max_mem, got, &calls)) { fprintf(stderr, "piece size %zu\n", piece); return 1; }
		if (got.size() != ref.size()) { fprintf(stderr, "piece size %zu: %zu members, expected %zu\n", piece, got.size(), ref.size()); return 1; }
		for (size_t k = 0; k < ref.size(); ++k)
			if (got[k].in_off != ref[k].in_off || got[k].out_off != ref[k].out_off || got[k].msize != ref[k].msize || got[k].isize != ref[k].isize) { fprintf(stderr, "piece size %zu: member %zu differs\n", piece, k); return 1; }
		++runs;
	}
	printf("san_bgzf_take: %zu members, largest %u bytes, %llu piece sizes, %llu takes\n", ref.size(), largest, (unsigned long long)runs, (unsigned long long)calls);
	return 0;
}

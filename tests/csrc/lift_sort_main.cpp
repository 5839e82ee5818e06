// lift_sort_main.cpp -- the order of `airlift-align lift --sorted` on the host, stand-alone under AddressSanitizer + UBSan (`make san-lift-sort`): the twin's
// compaction, descent count and stable sort (al_lift.h) and the run store -- add, chain, spill, merge, finish (al_run_store.h) -- host code only.
//
//   san_lift_sort LIST     LIST: one case per line, "<uncompressed BAM stream> <chain file>"
//
// Every case goes through the piece / carry loop in sorted mode at several piece sizes, and at each of them through a run store with limits from 1 byte upwards
// (1: a spill with every piece) and without a limit; every piece and every emitted chunk lies in a heap buffer of exactly its size.  At every combination the
// merged output must be in key order and hold the same bytes.  One line per case -- the counts, the descents of the whole stream, the largest number of spills
// and the FNV-1a hash of the sorted records -- then "san_lift_sort: N files".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fstream>
#include <string>
#include <vector>
#include "al_lift.h"
#include "al_run_store.h"

struct MemSource : AlLiftSource {
	const std::vector<uint8_t> *text = nullptr; size_t pos = 0; uint8_t *buf[2] = {nullptr, nullptr}; size_t n[2] = {0, 0}; bool at_eof[2] = {false, false};
	~MemSource() { free(buf[0]); free(buf[1]); }
	int read(int slot, size_t want) override
	{
		free(buf[slot]); buf[slot] = nullptr;
		n[slot] = std::min(want, text->size() - pos); at_eof[slot] = n[slot] < want;
		if (n[slot]) { buf[slot] = (uint8_t *)malloc(n[slot]); memcpy(buf[slot], text->data() + pos, n[slot]); pos += n[slot]; }
		return 0;
	}
	int push(AlLiftBackend &B, int slot, bool *eof) override { *eof = at_eof[slot]; return n[slot] ? B.append(slot, buf[slot], n[slot]) : 0; }
	size_t pending(int slot) const override { return n[slot]; }
};

static uint64_t fnv(uint64_t h, const void *p, size_t n) { const uint8_t *s = (const uint8_t *)p; for (size_t i = 0; i < n; ++i) { h ^= s[i]; h *= 0x100000001b3ull; } return h; }

int main(int argc, char **argv)
{
	if (argc < 2) { fprintf(stderr, "usage: san_lift_sort LIST\n"); return 2; }
	std::ifstream lst(argv[1]); std::string bam_fn, chain_fn; int n_files = 0;
	while (lst >> bam_fn >> chain_fn) {
		std::vector<uint8_t> text;
		{ std::ifstream f(bam_fn, std::ios::binary); text.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()); }
		AlLiftChain C; AlLiftHeader H; std::string err; size_t used = 0;
		if (al_lift_build(chain_fn.c_str(), C, err)) { printf("case %d refused=chain %s\n", n_files++, err.c_str()); continue; }
		if (al_lift_header_parse(text.data(), text.size(), H, &used, err) != 0) { printf("case %d refused=header %s\n", n_files++, err.c_str()); continue; }
		if (al_lift_bind(C, H, err)) { printf("case %d refused=bind %s\n", n_files++, err.c_str()); continue; }
		const std::vector<uint8_t> body(text.begin() + (ptrdiff_t)used, text.end());
		const size_t len = body.size() < 64 ? 64 : body.size();
		const size_t pieces[] = {64, 300, 1000, 4096, len}, limits[] = {1, 13, 2000, 20000, 0};
		size_t combos = 0; uint64_t h0 = 0, n0 = 0, max_spills = 0, whole_descents = 0; AlLiftRun st0;
		for (size_t piece : pieces) for (size_t limit : limits) {
			AlLiftHostBackend B(C.tab(), 1); B.set_sorted(true);
			MemSource src; src.text = &body; AlLiftRun st; AlRunStore store; store.limit = limit; std::string rows; uint64_t piece_descents = 0, n_pieces = 0;
			const int rc = al_lift_stream(B, src, piece, 0, used, bam_fn.c_str(), true, [&](int slot, const AlLiftPiece &r) -> int {
				const uint8_t *packed = nullptr, *arena = nullptr; const uint64_t *keys = nullptr; const uint32_t *lens = nullptr;
				if (B.finish(slot, &packed, &arena) || B.sorted_out(slot, &keys, &lens)) return -1;
				if (B.sort_launched(slot) != (r.descents != 0)) { fprintf(stderr, "a piece with %llu descents: sorted %d\n", (unsigned long long)r.descents, (int)B.sort_launched(slot)); return -1; }
				piece_descents += r.descents; ++n_pieces;
				// the store gets heap copies of exactly the arrays' sizes
				const size_t nk = (size_t)r.n_packed();
				uint8_t *pb = (uint8_t *)malloc((size_t)r.kept_bytes + 1); uint64_t *kb = (uint64_t *)malloc(nk * 8 + 8); uint32_t *lb = (uint32_t *)malloc(nk * 4 + 4);
				if (r.kept_bytes) memcpy(pb, packed, (size_t)r.kept_bytes);
				if (nk) { memcpy(kb, keys, nk * 8); memcpy(lb, lens, nk * 4); }
				const int ar = store.add_run(pb, (size_t)r.kept_bytes, kb, lb, nk);
				free(pb); free(kb); free(lb);
				al_lift_rows(arena, (size_t)r.arena_bytes, H, rows);
				return ar ? -1 : 0;
			}, st);
			if (rc) { fprintf(stderr, "%s: piece %zu limit %zu: al_lift_stream returned %d\n", bam_fn.c_str(), piece, limit, rc); return 1; }
			uint64_t h = 0xcbf29ce484222325ull, last = 0, n_out = 0; bool bad = false;
			const int fr = store.finish([&](const uint8_t *p, size_t n) {
				uint8_t *c = (uint8_t *)malloc(n); memcpy(c, p, n);
				for (size_t o = 0; o < n; ) {
					if (o + 36 > n) { bad = true; break; }
					const uint64_t k = al_lift_key(c + o); if (n_out && k < last) bad = true;
					last = k; ++n_out; o += 4 + (size_t)al_lift_u32(c + o);
					if (o > n) bad = true;
				}
				h = fnv(h, c, n); free(c);
				return bad ? 1 : 0; });
			if (fr || bad) { fprintf(stderr, "%s: piece %zu limit %zu: the merged output is not a sequence of whole records in key order (finish %d)\n", bam_fn.c_str(), piece, limit, fr); return 1; }
			h = fnv(h, rows.data(), rows.size());
			if (n_out != st.kept + st.unmapped_kept || store.records != n_out) { fprintf(stderr, "%s: piece %zu limit %zu: %llu records out, %llu kept\n", bam_fn.c_str(), piece, limit, (unsigned long long)n_out, (unsigned long long)(st.kept + st.unmapped_kept)); return 1; }
			if (limit == 1 && store.spills != store.runs_in) { fprintf(stderr, "%s: piece %zu: %llu spills of %llu runs at a limit of one byte\n", bam_fn.c_str(), piece, (unsigned long long)store.spills, (unsigned long long)store.runs_in); return 1; }
			if (limit == 0 && store.spills) { fprintf(stderr, "%s: piece %zu: a spill without a limit\n", bam_fn.c_str(), piece); return 1; }
			if (combos && (h != h0 || n_out != n0 || st.kept != st0.kept || st.unlifted != st0.unlifted)) { fprintf(stderr, "%s: piece %zu limit %zu: the output differs from the one before\n", bam_fn.c_str(), piece, limit); return 1; }
			h0 = h; n0 = n_out; st0 = st; ++combos;
			if (store.spills > max_spills) max_spills = store.spills;
			if (piece == len) whole_descents = piece_descents;                  // (the whole stream is one piece, and an empty one behind it)
		}
		printf("case %d combos=%zu kept=%llu unlifted=%llu unmapped=%llu descents=%llu spills=%llu fnv=%016llx\n", n_files, combos, (unsigned long long)st0.kept, (unsigned long long)st0.unlifted,
		       (unsigned long long)st0.unmapped_kept, (unsigned long long)whole_descents, (unsigned long long)max_spills, (unsigned long long)h0);
		++n_files;
	}
	printf("san_lift_sort: %d files\n", n_files);
	return 0;
}

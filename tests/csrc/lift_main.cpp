// lift_main.cpp -- the lift of `airlift-align lift` on the host, stand-alone under AddressSanitizer + UBSan (`make san-lift`): the block table's builder, the
// header's parser and writer, the kernels' twin (al_dev_lift.h) and the piece / carry loop (al_lift.h), host code only.
//
//   san_lift LIST     LIST: one case per line, "<uncompressed BAM stream> <chain file>"
//
// Every case is walked at every piece size from 64 bytes to 256, then at sizes growing by 1/16 up to the stream's length (every size of a stream of at most
// 4096 bytes), each piece from a heap buffer of exactly its size.  The counts, the packed records and the rows must be the same at every size.  One line per
// case -- the counts, or the code of a refusal -- then "san_lift: N files".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fstream>
#include <string>
#include <vector>
#include "al_lift.h"

// the stream's bytes from memory, every piece in a heap buffer of exactly its size (an overrun of a piece is an overrun of an allocation)
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
	if (argc < 2) { fprintf(stderr, "usage: san_lift LIST\n"); return 2; }
	std::ifstream lst(argv[1]); std::string bam_fn, chain_fn; int n_files = 0;
	while (lst >> bam_fn >> chain_fn) {
		std::vector<uint8_t> text;
		{ std::ifstream f(bam_fn, std::ios::binary); text.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()); }
		AlLiftChain C; AlLiftHeader H; std::string err; size_t used = 0;
		if (al_lift_build(chain_fn.c_str(), C, err)) { printf("case %d refused=chain %s\n", n_files++, err.c_str()); continue; }
		if (al_lift_header_parse(text.data(), text.size(), H, &used, err) != 0) { printf("case %d refused=header %s\n", n_files++, err.c_str()); continue; }
		if (al_lift_bind(C, H, err)) { printf("case %d refused=bind %s\n", n_files++, err.c_str()); continue; }
		std::vector<uint8_t> hdr; al_lift_header_write(H, C, hdr);
		const std::vector<uint8_t> body(text.begin() + (ptrdiff_t)used, text.end());
		size_t sizes = 0; int rc0 = 0; uint64_t h0 = 0; AlLiftRun st0;
		const size_t len = body.size() < 64 ? 64 : body.size();
		for (size_t piece = 64; ; ) {
			AlLiftHostBackend B(C.tab(), 1); MemSource src; src.text = &body; AlLiftRun st; uint64_t h = fnv(0xcbf29ce484222325ull, hdr.data(), hdr.size()); std::string rows;
			const int rc = al_lift_stream(B, src, piece, 0, used, bam_fn.c_str(), true, [&](int slot, const AlLiftPiece &r) -> int {
				const uint8_t *packed = nullptr, *arena = nullptr;
				if (B.finish(slot, &packed, &arena)) return -1;
				h = fnv(h, packed, (size_t)r.kept_bytes);
				al_lift_rows(arena, (size_t)r.arena_bytes, H, rows);
				return 0;
			}, st);
			h = fnv(h, rows.data(), rows.size());
			if (rc == -1) { fprintf(stderr, "%s: piece %zu: al_lift_stream failed\n", bam_fn.c_str(), piece); return 1; }
			if (sizes && (rc != rc0 || (rc == 0 && (h != h0 || st.kept != st0.kept || st.unlifted != st0.unlifted || st.unmapped_kept != st0.unmapped_kept)))) {
				fprintf(stderr, "%s: piece %zu: rc %d, %llu kept, %llu unlifted, %llu unmapped; before it rc %d, %llu, %llu, %llu (or the bytes differ)\n", bam_fn.c_str(), piece, rc,
				        (unsigned long long)st.kept, (unsigned long long)st.unlifted, (unsigned long long)st.unmapped_kept, rc0, (unsigned long long)st0.kept, (unsigned long long)st0.unlifted, (unsigned long long)st0.unmapped_kept);
				return 1;
			}
			rc0 = rc; h0 = h; st0 = st; ++sizes;
			if (piece >= len) break;
			const size_t next = (piece < 256 || len <= 4096) ? piece + 1 : piece + piece / 16;
			piece = next > len ? len : next;
		}
		if (rc0) printf("case %d sizes=%zu refused=%d\n", n_files, sizes, rc0);
		else printf("case %d sizes=%zu kept=%llu unlifted=%llu unmapped=%llu\n", n_files, sizes, (unsigned long long)st0.kept, (unsigned long long)st0.unlifted, (unsigned long long)st0.unmapped_kept);
		++n_files;
	}
	printf("san_lift: %d files\n", n_files);
	return 0;
}

// inflate_main.cpp -- the BGZF inflater's host twin (al_dev_inflate.h) as a stand-alone program for AddressSanitizer + UBSan (`make san-inflate`).
// Every file named in the list is read into a heap buffer of exactly its size and its members are listed along the BSIZE chain; every member is copied
// into a heap buffer of exactly its size and inflated into one of exactly ISIZE bytes (so a read or write past either end is seen), and the loop
// iterations the twin counted are held against the caps: 8 x csize input bits (+ the reader's slack) and ISIZE output bytes.
// usage: san_inflate LIST   (LIST: a file of file names, one per line)
// prints per file: "<name> chain=<0|-2> out=<bytes> crc=<CRC32 of all output, hex> st=<status,status,...>"; exit status 0 unless a cap was broken.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "al_dev_inflate.h"

int main(int argc, char **argv)
{
	if (argc != 2) { fprintf(stderr, "usage: %s LIST\n", argv[0]); return 2; }
	FILE *lf = fopen(argv[1], "r");
	if (!lf) { perror(argv[1]); return 2; }
	char line[4096]; size_t n_files = 0, n_members = 0;
	while (fgets(line, sizeof(line), lf)) {
		std::string fn(line);
		while (!fn.empty() && (fn.back() == '\n' || fn.back() == '\r')) fn.pop_back();
		if (fn.empty()) continue;
		FILE *f = fopen(fn.c_str(), "rb");
		if (!f) { perror(fn.c_str()); return 2; }
		fseek(f, 0, SEEK_END); const size_t n = (size_t)ftell(f); fseek(f, 0, SEEK_SET);
		uint8_t *buf = (uint8_t *)malloc(n ? n : 1);
		if (n && fread(buf, 1, n, f) != n) { perror(fn.c_str()); return 2; }
		fclose(f);
		std::vector<AlInfMember> mem; uint64_t pos = 0, out_n = 0;
		const int lr = al_inf_list(buf, n, &pos, &out_n, ~0ull, (size_t)-1, mem);
		const int chain = (lr != 0 || pos != n) ? -2 : 0;
		uint32_t reg = 0; uint64_t total = 0; std::string st;
		for (const AlInfMember &M : mem) {
			uint8_t *m = (uint8_t *)malloc(M.msize), *out = (uint8_t *)malloc(M.isize ? M.isize : 1);
			memcpy(m, buf + M.in_off, M.msize);
			uint64_t iters = 0;
			const int s = al_inflate_member_host(m, M.msize, out, &iters);
			if (iters > 8ull * M.msize + AL_INF_SLACK + M.isize + 8) { fprintf(stderr, "%s: member at %llu: %llu loop iterations for %u bytes in, %u out\n", fn.c_str(), (unsigned long long)M.in_off, (unsigned long long)iters, M.msize, M.isize); return 1; }
			if (s == 0) for (uint32_t i = 0; i < M.isize; ++i) { if (total == 0 && i == 0) reg = 0xffffffffu; reg = al_dfl_crc_byte(reg, out[i]); }
			if (s == 0) total += M.isize;
			st += (st.empty() ? "" : ",") + std::to_string(s);
			free(m); free(out); ++n_members;
		}
		printf("%s chain=%d out=%llu crc=%08x st=%s\n", fn.c_str(), chain, (unsigned long long)total, total ? ~reg : 0u, st.c_str());
		free(buf); ++n_files;
	}
	fclose(lf);
	printf("san_inflate: %zu files, %zu members\n", n_files, n_members);
	return 0;
}

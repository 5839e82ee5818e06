// regions_main.cpp -- the region merge of tokens --regions-bed / --merged-bed on the host, stand-alone under AddressSanitizer + UBSan (`make san-regions`):
// the fold's twin, the contig ranks and the BED formatter of al_dev_regions.h, host code only.
//
//   san_regions LIST     LIST: per case a line "case NAME N C K chunk_1 .. chunk_K", C lines of contig names (by contig index), N lines "group contig start end"
//
// Every case goes through al_regions_chunked_host at each of its chunk sizes, per gap and merged across the gaps, from a heap array of exactly its size.
// Printed per run: "== NAME chunk per_gap regions" and the BED text; at the end "san_regions: N cases".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <string>
#include <vector>
#include "al_dev_regions.h"

int main(int argc, char **argv)
{
	if (argc != 2) { fprintf(stderr, "usage: san_regions LIST\n"); return 2; }
	FILE *f = fopen(argv[1], "r");
	if (!f) { perror(argv[1]); return 2; }
	char name[256], buf[4096]; unsigned long long n = 0, c = 0, k = 0; int n_cases = 0;
	while (fscanf(f, " case %255s %llu %llu %llu", name, &n, &c, &k) == 4) {
		std::vector<unsigned long long> chunks(k);
		for (auto &x : chunks) if (fscanf(f, "%llu", &x) != 1) return 3;
		std::vector<std::string> names(c);
		for (auto &s : names) { if (fscanf(f, "%4095s", buf) != 1) return 3; s = buf; }
		std::vector<uint32_t> rank_of; std::vector<std::string> name_of;
		al_regions_ranks(names, rank_of, name_of);
		std::unique_ptr<AlRegIv[]> in(new AlRegIv[n]);                      // exactly n: an overrun of the input is an overrun of an allocation
		for (unsigned long long i = 0; i < n; ++i) {
			unsigned g, r, s, e;
			if (fscanf(f, "%u %u %u %u", &g, &r, &s, &e) != 4 || r >= c) return 3;
			in[i] = AlRegIv{g, rank_of[r], s, e};
		}
		for (unsigned long long chunk : chunks)
			for (int per_gap = 1; per_gap >= 0; --per_gap) {
				std::vector<AlRegIv> v;
				al_regions_chunked_host(in.get(), n, chunk, per_gap != 0, v);
				std::string text; al_regions_bed(text, v.data(), v.size(), name_of);
				printf("== %s %llu %d %zu\n", name, chunk, per_gap, v.size());
				fwrite(text.data(), 1, text.size(), stdout);
			}
		++n_cases;
	}
	fclose(f);
	printf("san_regions: %d cases\n", n_cases);
	return 0;
}

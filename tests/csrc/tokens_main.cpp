// tokens_main.cpp -- the tokens of `tokens --gaps-bed` on the host, stand-alone under AddressSanitizer + UBSan (`make san-tokens`): the BED row parser, the
// region table, the set-up kernel's twin, the runs of a batch and the SAM sink's names and bases of al_dev_tokens.h, host code only.
//
//   san_tokens LIST     LIST holds, line by line,
//     "case NAME R S SEED N"     then N lines "head src len": a table given directly
//     "bed NAME R S C L"         then C lines "contig length", then L raw BED lines: the table of a BED over contigs whose bases are the codes
//                                (p * 7 + p / 13) % 5 of their place p in the concatenated reference (4 = N)
//
// Printed per case: "== NAME rows tokens", the table ("T first_tok h_prefix" per row), and for chunks of 1, 7 and all tokens ("C chunk") every range's runs
// ("G t0 n first:row ...") and every token's "start hash", each range evaluated into heap arrays of exactly its size.  Per bed: "== NAME", per line
// "row LINE head contig start len", "skip LINE" or "err LINE why" -- after which the rest is not read and "refused" ends the block --, then the case output of its table, then per token "tok NAME START BASES".
// At the end "san_tokens: N cases".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <memory>
#include <string>
#include <vector>
#include "al_dev_tokens.h"

static void run_case(const char *name, const std::vector<std::string> &heads, const std::vector<uint64_t> &src, const std::vector<uint32_t> &len, int R, int S, int seed)
{
	std::vector<uint64_t> first_tok; std::vector<uint32_t> h_prefix;
	al_tok_table(heads, len.data(), R, S, first_tok, h_prefix);
	const uint32_t n_rows = (uint32_t)heads.size(); const uint64_t n_tok = first_tok[n_rows];
	printf("== %s %u %llu\n", name, n_rows, (unsigned long long)n_tok);
	for (uint32_t r = 0; r < n_rows; ++r) printf("T %llu %u\n", (unsigned long long)first_tok[r], h_prefix[r]);
	// the table as the kernel gets it: arrays of exactly their sizes
	std::unique_ptr<uint64_t[]> ft(new uint64_t[n_rows + 1]), sr(new uint64_t[n_rows]); std::unique_ptr<uint32_t[]> hp(new uint32_t[n_rows]);
	std::copy(first_tok.begin(), first_tok.end(), ft.get()); std::copy(src.begin(), src.end(), sr.get()); std::copy(h_prefix.begin(), h_prefix.end(), hp.get());
	const AlTokTab T{ft.get(), sr.get(), hp.get(), n_rows};
	for (uint64_t chunk : {(uint64_t)1, (uint64_t)7, (uint64_t)0}) {
		printf("C %llu\n", (unsigned long long)chunk);
		for (uint64_t t0 = 0; t0 < n_tok; ) {
			const uint64_t n = chunk ? std::min(chunk, n_tok - t0) : n_tok;
			std::unique_ptr<uint64_t[]> start(new uint64_t[n]); std::unique_ptr<uint32_t[]> hash(new uint32_t[n]);
			al_tok_setup_host(T, t0, n, R, S, seed, start.get(), hash.get());
			std::vector<uint32_t> g_first, g_id;
			al_tok_runs(ft.get(), n_rows, t0, n, g_first, g_id);
			printf("G %llu %llu", (unsigned long long)t0, (unsigned long long)n);
			for (size_t j = 0; j < g_id.size(); ++j) printf(" %u:%u", g_first[j], g_id[j]);
			printf("\n");
			for (uint64_t i = 0; i < n; ++i) printf("%llu %u\n", (unsigned long long)start[i], hash[i]);
			t0 += n;
		}
	}
}

int main(int argc, char **argv)
{
	if (argc != 2) { fprintf(stderr, "usage: san_tokens LIST\n"); return 2; }
	FILE *f = fopen(argv[1], "r");
	if (!f) { perror(argv[1]); return 2; }
	std::vector<char> line(1 << 16); char name[256], buf[4096]; int n_cases = 0;
	auto next_line = [&]() -> bool { return fgets(line.data(), (int)line.size(), f) != nullptr; };
	while (next_line()) {
		int R = 0, S = 0, seed = 0; unsigned long long n = 0, c = 0;
		if (sscanf(line.data(), "case %255s %d %d %d %llu", name, &R, &S, &seed, &n) == 5) {
			std::vector<std::string> heads; std::vector<uint64_t> src; std::vector<uint32_t> len;
			for (unsigned long long i = 0; i < n; ++i) {
				unsigned long long s; unsigned l;
				if (!next_line() || sscanf(line.data(), "%4095s %llu %u", buf, &s, &l) != 3) return 3;
				heads.push_back(buf); src.push_back(s); len.push_back(l);
			}
			run_case(name, heads, src, len, R, S, seed);
		} else if (sscanf(line.data(), "bed %255s %d %d %llu %llu", name, &R, &S, &c, &n) == 5) {
			std::vector<std::string> cn; std::vector<uint32_t> cl; std::vector<uint64_t> co; uint64_t tot = 0;
			for (unsigned long long i = 0; i < c; ++i) {
				unsigned l;
				if (!next_line() || sscanf(line.data(), "%4095s %u", buf, &l) != 2) return 3;
				cn.push_back(buf); cl.push_back(l); co.push_back(tot); tot += l;
			}
			std::unique_ptr<uint32_t[]> S4(new uint32_t[(tot + 7) / 8 + 1]());                 // a window's last base is inside: no padding is read here
			for (uint64_t p = 0; p < tot; ++p) S4[p >> 3] |= (uint32_t)((p * 7 + p / 13) % 5) << ((p & 7) << 2);
			auto contig = [&](const std::string &nm, uint32_t *clen) -> int64_t { for (size_t i = 0; i < cn.size(); ++i) if (cn[i] == nm) { *clen = cl[i]; return (int64_t)i; } return -1; };
			printf("== %s\n", name);
			std::vector<std::string> heads; std::vector<uint64_t> src; std::vector<uint32_t> len; bool refused = false;
			for (unsigned long long i = 1; i <= n; ++i) {
				if (!next_line()) return 3;
				if (refused) continue;                                            // (the run ends at the first refused row)
				const size_t l = strlen(line.data());
				std::unique_ptr<char[]> exact(new char[l ? l : 1]); memcpy(exact.get(), line.data(), l);      // exactly the line's bytes, no terminator
				AlTokRow row; const char *why = nullptr;
				const int r = al_tok_parse_row(exact.get(), l, contig, row, &why);
				if (r < 0) { printf("err %llu %s\n", i, why); refused = true; continue; }
				if (r > 0) { printf("skip %llu\n", i); continue; }
				printf("row %llu %s %u %u %u\n", i, row.head.c_str(), row.rid, row.start, row.len);
				heads.push_back(row.head); src.push_back(co[row.rid] + row.start); len.push_back(row.len);
			}
			if (refused) { printf("refused\n"); ++n_cases; continue; }
			run_case(name, heads, src, len, R, S, 11);
			std::vector<uint64_t> first_tok; std::vector<uint32_t> h_prefix;
			al_tok_table(heads, len.data(), R, S, first_tok, h_prefix);
			std::string nm; std::unique_ptr<char[]> bases(new char[R]);
			for (uint64_t t = 0; t < first_tok[heads.size()]; ++t) {
				const uint32_t r = al_tok_row(first_tok.data(), (uint32_t)heads.size(), t), off = (uint32_t)(t - first_tok[r]) * (uint32_t)S;
				al_tok_name(heads[r], off, nm); al_tok_bases(S4.get(), src[r] + off, R, bases.get());
				printf("tok %s %llu %.*s\n", nm.c_str(), (unsigned long long)(src[r] + off), R, bases.get());
			}
		} else if (line[0] != '\n') return 3;
		else continue;
		++n_cases;
	}
	fclose(f);
	printf("san_tokens: %d cases\n", n_cases);
	return 0;
}

// chainreg_main.cpp -- the chain file's region logic of chain-beds / tokens --chain on the host, stand-alone under AddressSanitizer + UBSan (`make san-chainreg`):
// the parser of the chain file and of the merged BED, the kernels' twin and the BED formatter of al_dev_chainreg.h, host code only.
//
//   san_chainreg LIST     LIST: per case a line "NAME R E CHAIN MERGED" (MERGED "-": no retired step)
//
// Every case is parsed, evaluated by the twin from heap arrays of exactly its size, and printed: "== NAME gaps|constant|retired ROWS" and the BED text, or
// "== NAME refused" and the parser's message for a file it refuses; at the end "san_chainreg: N cases".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <string>
#include <vector>
#include "al_dev_chainreg.h"

int main(int argc, char **argv)
{
	if (argc != 2) { fprintf(stderr, "usage: san_chainreg LIST\n"); return 2; }
	FILE *f = fopen(argv[1], "r");
	if (!f) { perror(argv[1]); return 2; }
	char name[256], chain[4096], merged[4096]; int R = 0, E = 0, n_cases = 0;
	while (fscanf(f, " %255s %d %d %4095s %4095s", name, &R, &E, chain, merged) == 5) {
		++n_cases;
		const bool ret = strcmp(merged, "-") != 0;
		AlChnTab tab; AlChnRet r; std::string err;
		if (al_chn_parse(chain, tab, err) != 0 || (ret && al_chn_parse_merged(merged, tab, r, err) != 0)) { printf("== %s refused\n%s\n", name, err.c_str()); continue; }
		// exactly-sized copies of every array: an overrun of the input is an overrun of an allocation
		const size_t n = tab.line.size(), nc = tab.c_slot.size(), ns = tab.L.size(), nm = r.M.size(), nr = r.L.size();
		std::unique_ptr<AlChnLine[]> line(new AlChnLine[n]); std::unique_ptr<uint32_t[]> c_slot(new uint32_t[nc]), c_tstart(new uint32_t[nc]), L(new uint32_t[ns]), rslot_of(new uint32_t[ns]), RL(new uint32_t[nr]);
		std::unique_ptr<AlChnIv[]> M(new AlChnIv[nm]);
		std::copy(tab.line.begin(), tab.line.end(), line.get()); std::copy(tab.c_slot.begin(), tab.c_slot.end(), c_slot.get()); std::copy(tab.c_tstart.begin(), tab.c_tstart.end(), c_tstart.get());
		std::copy(tab.L.begin(), tab.L.end(), L.get()); std::copy(r.M.begin(), r.M.end(), M.get()); std::copy(r.L.begin(), r.L.end(), RL.get());
		if (ret) std::copy(r.rslot_of.begin(), r.rslot_of.end(), rslot_of.get());
		AlChnIn in; in.n = n; in.line = line.get(); in.n_chain = (uint32_t)nc; in.c_slot = c_slot.get(); in.c_tstart = c_tstart.get(); in.n_slot = (uint32_t)ns; in.L = L.get();
		if (ret) { in.n_m = nm; in.M = M.get(); in.n_rslot = (uint32_t)nr; in.rslot_of = rslot_of.get(); in.RL = RL.get(); }
		const char *why = al_chn_in_bad(in, ret);
		if (why) { printf("== %s broken\n%s\n", name, why); continue; }
		std::vector<AlChnIv> g, c, t;
		al_chainreg_host(in, R, E, &g, &c, ret ? &t : nullptr);
		std::string text;
		auto put = [&](const char *kind, const std::vector<AlChnIv> &v, const std::vector<std::string> &names) {
			text.clear(); al_chn_bed(text, v.data(), v.size(), names);
			printf("== %s %s %zu\n", name, kind, v.size());
			fwrite(text.data(), 1, text.size(), stdout);
		};
		put("gaps", g, tab.name); put("constant", c, tab.name);
		if (ret) put("retired", t, r.name);
	}
	fclose(f);
	printf("san_chainreg: %d cases\n", n_cases);
	return 0;
}

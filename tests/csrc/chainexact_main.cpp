// chainexact_main.cpp -- chain-exact verify|build on the host, stand-alone under AddressSanitizer + UBSan (`make san-chainexact`): the chain file's parser,
// the table builder, the kernels' twin, pass 3 and the printing of al_dev_chainexact.h, host code only.
//
//   san_chainexact LIST     LIST: per case a line "NAME MODE M OLD.fa NEW.fa CHAIN" (MODE verify | build, M the smallest region)
//
// Every case is read, evaluated by the twin from heap arrays of exactly its size, and printed: "== NAME MODE BYTES" and the text, or "== NAME refused" and the
// message; at the end "san_chainexact: N cases".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <string>
#include <vector>
#include "al_dev_chainexact.h"

// a plain FASTA: the name ends at the first blank, the lines of a record joined as they are; the text in an allocation of exactly its size
static bool read_fa(const char *fn, AlCexFa &fa, std::unique_ptr<uint8_t[]> &text)
{
	AlChnLineReader rd;
	if (!rd.open(fn)) return false;
	std::string all; const char *l; size_t n;
	while (rd.next(&l, &n)) {
		while (n && (l[n - 1] == '\n' || l[n - 1] == '\r')) --n;
		if (n && l[0] == '>') {
			size_t e = 1; while (e < n && l[e] != ' ' && l[e] != '\t') ++e;
			fa.name.push_back(std::string(l + 1, e - 1)); fa.off.push_back(all.size()); fa.len.push_back(0);
		} else if (!fa.name.empty()) { all.append(l, n); fa.len.back() += (uint32_t)n; }
	}
	text.reset(new uint8_t[all.size()]);
	memcpy(text.get(), all.data(), all.size());
	fa.text = text.get(); fa.n = all.size();
	return true;
}

int main(int argc, char **argv)
{
	if (argc != 2) { fprintf(stderr, "usage: san_chainexact LIST\n"); return 2; }
	FILE *f = fopen(argv[1], "r");
	if (!f) { perror(argv[1]); return 2; }
	char name[256], mode_s[16], old_fn[4096], new_fn[4096], chain[4096]; int M = 0, n_cases = 0;
	while (fscanf(f, " %255s %15s %d %4095s %4095s %4095s", name, mode_s, &M, old_fn, new_fn, chain) == 6) {
		++n_cases;
		const int mode = strcmp(mode_s, "build") ? AL_CEX_VERIFY : AL_CEX_BUILD;
		AlCexTab tab; AlCexFa fo, fn; std::unique_ptr<uint8_t[]> to, tn; std::string err; AlCexRun run;
		if (!read_fa(old_fn, fo, to) || !read_fa(new_fn, fn, tn)) { printf("== %s unreadable\n", name); continue; }
		const std::string *twice = fo.index(); if (!twice) twice = fn.index();
		if (twice) { printf("== %s refused\ncontig '%s' twice\n", name, twice->c_str()); continue; }
		if (al_cex_parse(chain, tab, err) != 0 || al_cex_table(chain, tab, fo, fn, mode, run, err) != 0) { printf("== %s refused\n%s\n", name, err.c_str()); continue; }
		// exactly-sized copies of the tables: an overrun of the input is an overrun of an allocation
		const size_t n = run.line.size(), nc = run.chain.size();
		std::unique_ptr<AlCexLine[]> line(new AlCexLine[n]); std::unique_ptr<AlCexChain[]> ch(new AlCexChain[nc]);
		std::copy(run.line.begin(), run.line.end(), line.get()); std::copy(run.chain.begin(), run.chain.end(), ch.get());
		AlCexIn in; in.old_text = fo.text; in.n_old = fo.n; in.new_text = fn.text; in.n_new = fn.n; in.n = n; in.line = line.get(); in.n_chain = (uint32_t)nc; in.chain = ch.get();
		const char *why = al_cex_in_bad(in, mode == AL_CEX_BUILD);
		if (why) { printf("== %s broken\n%s\n", name, why); continue; }
		AlCexOut o;
		al_chainexact_host(in, mode == AL_CEX_BUILD, (uint32_t)M, o);
		if (o.flag) { printf("== %s refused\n%s:%llu: a byte other than acgtnACGTN\n", name, chain, al_cex_flag_line(in, run)); continue; }
		std::string text;
		if (mode == AL_CEX_BUILD) al_cex_build_text(tab, o.lines2, text); else al_cex_verify_text(tab, run, o.cnt, text);
		printf("== %s %s %zu\n", name, mode_s, text.size());
		fwrite(text.data(), 1, text.size(), stdout);
	}
	fclose(f);
	printf("san_chainexact: %d cases\n", n_cases);
	return 0;
}

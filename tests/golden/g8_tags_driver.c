/* TEST INFRASTRUCTURE ONLY -- driver for tests/golden/make_g8_tags.py.  Our own code, linked against the fork compiled where it lies
 * (map.c with the ALSER early return removed, as oracle/Makefile does), through its public minimap.h API: `-ax sr` mapping of one or
 * two read files to SAM on stdout with the output options of the fork's command line (main.c:164, 207, 210, 223-233) taken from argv.
 * usage: g8drv [-R rgline] [--MD] [--cs[=short|long|none]] [--eqx] [-Y] ref.fa r1 [r2] */
#include <stdio.h>
#include <string.h>
#include "minimap.h"

int main(int argc, char **argv)
{
	mm_idxopt_t io; mm_mapopt_t mo; mm_idx_reader_t *r; mm_idx_t *mi;
	const char *rg = 0, *fn[4]; int i, nfn = 0;
	mm_set_opt(0, &io, &mo); mm_set_opt("sr", &io, &mo);
	mo.flag |= MM_F_OUT_SAM | MM_F_CIGAR;
	for (i = 1; i < argc; ++i) {
		if (!strcmp(argv[i], "-R") && i + 1 < argc) rg = argv[++i];
		else if (!strcmp(argv[i], "--MD")) mo.flag |= MM_F_OUT_MD;
		else if (!strcmp(argv[i], "--eqx")) mo.flag |= MM_F_EQX;
		else if (!strcmp(argv[i], "-Y")) mo.flag |= MM_F_SOFTCLIP;
		else if (!strncmp(argv[i], "--cs", 4)) {
			const char *v = argv[i][4] == '=' ? argv[i] + 5 : 0;
			mo.flag |= MM_F_OUT_CS | MM_F_CIGAR;
			if (!v || !strcmp(v, "short")) mo.flag &= ~MM_F_OUT_CS_LONG;
			else if (!strcmp(v, "long")) mo.flag |= MM_F_OUT_CS_LONG;
			else if (!strcmp(v, "none")) mo.flag &= ~MM_F_OUT_CS;
		} else if (nfn < 4) fn[nfn++] = argv[i];
	}
	if (nfn < 2 || mm_check_opt(&io, &mo) < 0) { fprintf(stderr, "usage: g8drv [opts] ref.fa r1 [r2]\n"); return 2; }
	if ((r = mm_idx_reader_open(fn[0], &io, 0)) == 0) return 1;
	while ((mi = mm_idx_reader_read(r, 1)) != 0) {
		mm_mapopt_update(&mo, mi);
		mm_write_sam_hdr(mi, rg, 0, 0, 0);
		if (nfn == 2 && !(mo.flag & MM_F_FRAG_MODE)) mm_map_file(mi, fn[1], &mo, 1);
		else mm_map_file_frag(mi, nfn - 1, &fn[1], &mo, 1);
		mm_idx_destroy(mi);
	}
	mm_idx_reader_close(r);
	fflush(stdout);
	return 0;
}

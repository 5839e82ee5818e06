/* TEST INFRASTRUCTURE ONLY -- driver for tests/golden/make_g9_paf.py.  Our own code, linked against the fork compiled where it lies
 * (map.c with the ALSER early return removed, as oracle/Makefile does), through its public minimap.h API: `-x sr` mapping of one or
 * two read files to stdout.  As the fork's command line (main.c:158, 211, 213-222) the default output is PAF without base-level
 * alignment; -a selects SAM, -c / --cs turn the alignment on.
 * usage: g9drv [-a] [-c] [-R rgline] [--MD] [--cs[=short|long|none]] [--eqx] [-Y] [--paf-no-hit] [--secondary=yes|no] ref.fa r1 [r2] */
#include <stdio.h>
#include <string.h>
#include "minimap.h"

int main(int argc, char **argv)
{
	mm_idxopt_t io; mm_mapopt_t mo; mm_idx_reader_t *r; mm_idx_t *mi;
	const char *rg = 0, *fn[4]; int i, nfn = 0;
	mm_set_opt(0, &io, &mo); mm_set_opt("sr", &io, &mo);
	for (i = 1; i < argc; ++i) {
		if (!strcmp(argv[i], "-R") && i + 1 < argc) rg = argv[++i];
		else if (!strcmp(argv[i], "-a")) mo.flag |= MM_F_OUT_SAM | MM_F_CIGAR;
		else if (!strcmp(argv[i], "-c")) mo.flag |= MM_F_OUT_CG | MM_F_CIGAR;
		else if (!strcmp(argv[i], "--MD")) mo.flag |= MM_F_OUT_MD;
		else if (!strcmp(argv[i], "--eqx")) mo.flag |= MM_F_EQX;
		else if (!strcmp(argv[i], "-Y")) mo.flag |= MM_F_SOFTCLIP;
		else if (!strcmp(argv[i], "--paf-no-hit")) mo.flag |= MM_F_PAF_NO_HIT;
		else if (!strcmp(argv[i], "--secondary=yes")) mo.flag &= ~MM_F_NO_PRINT_2ND;
		else if (!strcmp(argv[i], "--secondary=no")) mo.flag |= MM_F_NO_PRINT_2ND;
		else if (!strncmp(argv[i], "--cs", 4)) {
			const char *v = argv[i][4] == '=' ? argv[i] + 5 : 0;
			mo.flag |= MM_F_OUT_CS | MM_F_CIGAR;
			if (!v || !strcmp(v, "short")) mo.flag &= ~MM_F_OUT_CS_LONG;
			else if (!strcmp(v, "long")) mo.flag |= MM_F_OUT_CS_LONG;
			else if (!strcmp(v, "none")) mo.flag &= ~MM_F_OUT_CS;
		} else if (nfn < 4) fn[nfn++] = argv[i];
	}
	if (nfn < 2 || mm_check_opt(&io, &mo) < 0) { fprintf(stderr, "usage: g9drv [opts] ref.fa r1 [r2]\n"); return 2; }
	if ((r = mm_idx_reader_open(fn[0], &io, 0)) == 0) return 1;
	while ((mi = mm_idx_reader_read(r, 1)) != 0) {
		mm_mapopt_update(&mo, mi);
		if (mo.flag & MM_F_OUT_SAM) mm_write_sam_hdr(mi, rg, 0, 0, 0);
		if (nfn == 2 && !(mo.flag & MM_F_FRAG_MODE)) mm_map_file(mi, fn[1], &mo, 1);
		else mm_map_file_frag(mi, nfn - 1, &fn[1], &mo, 1);
		mm_idx_destroy(mi);
	}
	mm_idx_reader_close(r);
	fflush(stdout);
	return 0;
}

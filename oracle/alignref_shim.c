/* TEST INFRASTRUCTURE ONLY -- the reference's path from a fragment's chains to its final records, callable fragment by fragment
 * (oracle/_ref/libalignref.so, see oracle/Makefile).
 *
 * This file is OUR code and holds none of the reference's.  The Makefile compiles it with -I$(REF) beside the fork's sources where they lie;
 * everything called here is declared in the fork's minimap.h and mmpriv.h.  alignref_frag() runs what mm_map_frag runs from mm_gen_regs to
 * mm_pair (map.c:379-405) under `-ax sr` on the caller's chains, on a real mm_idx_t made by mm_idx_str:
 *   mm_gen_regs, chain_post (mm_set_parent, mm_select_sub / mm_select_sub_multi), for a pair mm_seg_gen and the per-mate mm_set_parent,
 *   per mate align_regs -- static in map.c, so restated here: mm_align_skeleton, mm_set_parent, mm_select_sub, mm_set_sam_pri -- and mm_set_mapq,
 *   for a pair mm_pair.
 * The mates' sequences come in mapping orientation (mate 2 already flipped, as worker_for hands them on).
 * A record is ALIGNREF_NF int32 words:
 *   id parent score score0 cnt rid qs qe rs re subsc n_sub hash mlen blen mapq rev split inv split_inv proper_frag pe_thru sam_pri seg_split seg_id
 *   has_p dp_score dp_max dp_max2 n_ambi trans_strand n_cigar
 * and its CIGAR words follow one another in cig[], record after record.  `div` is left out (sr never computes it).
 * The fork asserts its preconditions (align.c:600, 686, 707, 725, 772, 778): frag_check() refuses beforehand what would trip them. */
#include <stdlib.h>
#include <string.h>
#include "minimap.h"
#include "mmpriv.h"
#include "frag_check.h"

#define ALIGNREF_NF 32
#define ALIGNREF_NI 21       /* iopt: k bw max_gap max_gap_ref max_frag_len min_cnt min_chain_score best_n a b q e q2 e2 sc_ambi zdrop zdrop_inv end_bonus min_dp_max pe_ori pe_bonus */

int alignref_nf(void) { return ALIGNREF_NF; }
int alignref_ni(void) { return ALIGNREF_NI; }

void *alignref_idx(int w, int k, int n, const char **seqs, const char **names) { return mm_idx_str(w, k, 0, 14, n, seqs, names); }
void alignref_idx_free(void *mi) { if (mi) mm_idx_destroy((mm_idx_t*)mi); }

static void put(int32_t *o, const mm_reg1_t *r)
{
	o[0] = r->id; o[1] = r->parent; o[2] = r->score; o[3] = r->score0; o[4] = r->cnt; o[5] = r->rid; o[6] = r->qs; o[7] = r->qe; o[8] = r->rs; o[9] = r->re;
	o[10] = r->subsc; o[11] = r->n_sub; o[12] = (int32_t)r->hash; o[13] = r->mlen; o[14] = r->blen; o[15] = r->mapq; o[16] = r->rev; o[17] = r->split; o[18] = r->inv;
	o[19] = r->split_inv; o[20] = r->proper_frag; o[21] = r->pe_thru; o[22] = r->sam_pri; o[23] = r->seg_split; o[24] = r->seg_id; o[25] = r->p != 0;
	o[26] = r->p? r->p->dp_score : 0; o[27] = r->p? r->p->dp_max : 0; o[28] = r->p? r->p->dp_max2 : 0; o[29] = r->p? (int32_t)r->p->n_ambi : 0;
	o[30] = r->p? (int32_t)r->p->trans_strand : 0; o[31] = r->p? (int32_t)r->p->n_cigar : 0;
}

/* align_regs of map.c:260-270 with MM_F_CIGAR set and MM_F_ALL_CHAINS clear, in our words */
static mm_reg1_t *align_mate(const mm_mapopt_t *opt, const mm_idx_t *mi, int qlen, const char *seq, int *n, mm_reg1_t *r, mm128_t *a)
{
	r = mm_align_skeleton(0, opt, mi, qlen, seq, n, r, a);
	mm_set_parent(0, opt->mask_level, *n, r, opt->a * 2 + opt->b, 0);
	mm_select_sub(0, opt->pri_ratio, mi->k * 2, opt->best_n, n, r);
	mm_set_sam_pri(*n, r);
	return r;
}

/* u[n_u] = score << 32 | count, a_xy = the chains' anchors one chain after the other ((x, y) pairs, n_a of them).  out: max_hits records of room per
 * mate, mate s from record s * max_hits on; cig: max_cig words per mate, mate s from word s * max_cig on; n_hits[2], n_cigw[2].
 * Returns 0; < 0 from frag_check(); -20: a sequence is missing; -21 / -22: more hits / CIGAR words than there is room for. */
int alignref_frag(const void *mi_, const int32_t *io, const float *fo, int n_u, const uint64_t *u_in, const uint64_t *a_xy, int64_t n_a, uint32_t hash,
                  int n_segs, const int *qlens, const char **seqs, int rep_len, int max_hits, int max_cig, int32_t *n_hits, int32_t *out, int32_t *n_cigw, uint32_t *cig)
{
	const mm_idx_t *mi = (const mm_idx_t*)mi_;
	mm_idxopt_t iopt; mm_mapopt_t opt;
	int i, s, rc, qlen_sum = 0, n_regs0 = n_u, n_regs[2] = {0, 0}, max_gap_ref;
	int64_t j; uint32_t *lens;
	uint64_t *u; mm128_t *a; mm_reg1_t *regs0, *regs[2] = {0, 0};

	lens = (uint32_t*)malloc((mi->n_seq? mi->n_seq : 1) * 4);
	for (i = 0; i < (int)mi->n_seq; ++i) lens[i] = mi->seq[i].len;
	rc = frag_check(n_u, u_in, a_xy, n_a, n_segs, qlens, mi->n_seq, lens);
	free(lens);
	if (rc) return rc;
	for (s = 0; s < n_segs; ++s) { if (!seqs[s] || (int)strlen(seqs[s]) != qlens[s]) return -20; qlen_sum += qlens[s]; }

	mm_set_opt(0, &iopt, &opt); mm_set_opt("sr", &iopt, &opt);
	opt.flag |= MM_F_CIGAR | MM_F_OUT_SAM;
	if (mi->k != io[0]) return -20;
	opt.bw = io[1]; opt.max_gap = io[2]; opt.max_gap_ref = io[3]; opt.max_frag_len = io[4]; opt.min_cnt = io[5]; opt.min_chain_score = io[6]; opt.best_n = io[7];
	opt.a = io[8]; opt.b = io[9]; opt.q = io[10]; opt.e = io[11]; opt.q2 = io[12]; opt.e2 = io[13]; opt.sc_ambi = io[14]; opt.zdrop = io[15]; opt.zdrop_inv = io[16];
	opt.end_bonus = io[17]; opt.min_dp_max = io[18]; opt.pe_ori = io[19]; opt.pe_bonus = io[20];
	opt.mask_level = fo[0]; opt.pri_ratio = fo[1]; opt.max_clip_ratio = fo[2];
	if (opt.max_gap_ref > 0) max_gap_ref = opt.max_gap_ref;                                  /* map.c:344-349 */
	else if (opt.max_frag_len > 0) { max_gap_ref = opt.max_frag_len - qlen_sum; if (max_gap_ref < opt.max_gap) max_gap_ref = opt.max_gap; }
	else max_gap_ref = opt.max_gap;

	u = (uint64_t*)malloc((n_u > 0? n_u : 1) * 8);
	a = (mm128_t*)malloc((n_a > 0? n_a : 1) * 16);
	for (i = 0; i < n_u; ++i) u[i] = u_in[i];
	for (j = 0; j < n_a; ++j) a[j].x = a_xy[2 * j], a[j].y = a_xy[2 * j + 1];
	n_hits[0] = n_hits[1] = 0; n_cigw[0] = n_cigw[1] = 0;

	regs0 = mm_gen_regs(0, hash, qlen_sum, n_u, u, a);                                       /* map.c:379 */
	mm_set_parent(0, opt.mask_level, n_regs0, regs0, opt.a * 2 + opt.b, 0);                  /* chain_post */
	if (n_segs <= 1) mm_select_sub(0, opt.pri_ratio, mi->k * 2, opt.best_n, &n_regs0, regs0);
	else mm_select_sub_multi(0, opt.pri_ratio, 0.2f, 0.7f, max_gap_ref, mi->k * 2, opt.best_n, n_segs, qlens, &n_regs0, regs0);
	if (n_segs == 1) {                                                                       /* map.c:390-393 */
		regs0 = align_mate(&opt, mi, qlens[0], seqs[0], &n_regs0, regs0, a);
		mm_set_mapq(0, n_regs0, regs0, opt.min_chain_score, opt.a, rep_len, 1);
		n_regs[0] = n_regs0, regs[0] = regs0;
	} else {                                                                                 /* map.c:394-405 */
		mm_seg_t *seg = mm_seg_gen(0, hash, n_segs, qlens, n_regs0, regs0, n_regs, regs, a);
		free(regs0);
		for (s = 0; s < n_segs; ++s) {
			mm_set_parent(0, opt.mask_level, n_regs[s], regs[s], opt.a * 2 + opt.b, 0);
			regs[s] = align_mate(&opt, mi, qlens[s], seqs[s], &n_regs[s], regs[s], seg[s].a);
			mm_set_mapq(0, n_regs[s], regs[s], opt.min_chain_score, opt.a, rep_len, 1);
		}
		mm_seg_free(0, n_segs, seg);
		if (opt.pe_ori >= 0) mm_pair(0, max_gap_ref, opt.pe_bonus, opt.a * 2 + opt.b, opt.a, qlens, n_regs, regs);
	}
	rc = 0;
	for (s = 0; s < n_segs; ++s) {
		int k = 0;
		if (n_regs[s] > max_hits) rc = -21;
		for (i = 0; i < n_regs[s] && !rc; ++i) {
			const mm_reg1_t *r = &regs[s][i];
			put(out + ((size_t)s * max_hits + i) * ALIGNREF_NF, r);
			if (r->p) {
				if (k + (int)r->p->n_cigar > max_cig) { rc = -22; break; }
				memcpy(cig + (size_t)s * max_cig + k, r->p->cigar, (size_t)r->p->n_cigar * 4); k += r->p->n_cigar;
			}
		}
		n_hits[s] = n_regs[s]; n_cigw[s] = k;
		for (i = 0; i < n_regs[s]; ++i) free(regs[s][i].p);
		free(regs[s]);
	}
	free(u); free(a);
	return rc;
}

/* TEST INFRASTRUCTURE ONLY -- the reference's path from a fragment's chains to its per-mate hits, callable fragment by fragment
 * (oracle/_ref/libhitref.so, see oracle/Makefile).
 *
 * This file is OUR code and holds none of the reference's.  The Makefile compiles it with -I$(REF) beside the fork's hit.c, pe.c, misc.c and
 * kalloc.c where they lie; everything called here is declared in the fork's mmpriv.h.  hitref_frag() runs what mm_map_frag runs between
 * mm_chain_dp and mm_pair (map.c:379-403) when align_regs returns at once (no MM_F_CIGAR), under `-x sr` (no MM_F_ALL_CHAINS, no
 * mm_join_long, no hard mask level, is_sr = 1), on the caller's chains:
 *   A  after chain_post: the fragment-level hits; pre[] = (parent, as) of every hit between mm_set_parent and the selection
 *   B  the stage product: per mate the hits after mm_seg_gen and the per-mate mm_set_parent, and every hit's anchors (single end: A's hits)
 *   C  B's hits after mm_set_mapq
 * A hit is HITREF_NF int32 words: id parent score score0 cnt rid qs qe rs re subsc n_sub hash mlen blen rev sam_pri seg_split seg_id mapq
 * other as, `other` being every remaining flag bit (split, inv, proper_frag, pe_thru, split_inv) or'ed together.
 */
#include <stdlib.h>
#include <string.h>
#include "minimap.h"
#include "mmpriv.h"

#define HITREF_NF 22

int hitref_nf(void) { return HITREF_NF; }

static void put(int32_t *o, const mm_reg1_t *r)
{
	o[0] = r->id; o[1] = r->parent; o[2] = r->score; o[3] = r->score0; o[4] = r->cnt; o[5] = r->rid; o[6] = r->qs; o[7] = r->qe; o[8] = r->rs; o[9] = r->re;
	o[10] = r->subsc; o[11] = r->n_sub; o[12] = (int32_t)r->hash; o[13] = r->mlen; o[14] = r->blen; o[15] = r->rev; o[16] = r->sam_pri; o[17] = r->seg_split;
	o[18] = r->seg_id; o[19] = r->mapq; o[20] = r->split | r->inv << 2 | r->proper_frag << 3 | r->pe_thru << 4 | r->split_inv << 5 | (r->p != 0) << 6; o[21] = r->as;
}

/* B and C of one mate: n hits r[] over the anchors a[]; the hits' anchors go to anch (hit after hit), the count of them is returned */
static int64_t mate(int n, mm_reg1_t *r, mm128_t *a, int min_chain_sc, int match_sc, int rep_len, int32_t *B, int32_t *C, uint64_t *anch)
{
	int i, j; int64_t k = 0;
	mm_squeeze_a(0, n, r, a);
	for (i = 0; i < n; ++i) {
		put(B + (size_t)i * HITREF_NF, &r[i]);
		for (j = 0; j < r[i].cnt; ++j, ++k) anch[2 * k] = a[r[i].as + j].x, anch[2 * k + 1] = a[r[i].as + j].y;
	}
	mm_set_mapq(0, n, r, min_chain_sc, match_sc, rep_len, 1);
	for (i = 0; i < n; ++i) put(C + (size_t)i * HITREF_NF, &r[i]);
	return k;
}

/* u[n_u] = score << 32 | count, a_xy = the chains' anchors one chain after the other ((x, y) pairs, n_a of them).  A: n_u hits of room; pre: 2 n_u
 * words; B and C: n_u hits of room per mate, mate s from hit s * n_u on; anch: n_a pairs, mate 0's then mate 1's.  nB[2], n_anch[2]. */
int hitref_frag(int n_u, const uint64_t *u_in, const uint64_t *a_xy, int64_t n_a, uint32_t hash, int n_segs, const int *qlens, int rep_len,
                float mask_level, float pri_ratio, int best_n, int min_diff, int max_gap_ref, int sub_diff, int min_chain_sc, int match_sc,
                int32_t *pre, int32_t *nA, int32_t *A, int32_t *nB, int32_t *B, int32_t *C, uint64_t *anch, int64_t *n_anch)
{
	int i, s, qlen_sum = 0, n_regs0 = n_u, n_regs[2] = {0, 0};
	int64_t j;
	uint64_t *u; mm128_t *a; mm_reg1_t *regs0, *regs[2] = {0, 0};
	if (n_segs < 1 || n_segs > 2) return -1;
	for (i = 0; i < n_segs; ++i) qlen_sum += qlens[i];
	u = (uint64_t*)malloc((n_u > 0? n_u : 1) * 8);
	a = (mm128_t*)malloc((n_a > 0? n_a : 1) * 16);
	for (i = 0; i < n_u; ++i) u[i] = u_in[i];
	for (j = 0; j < n_a; ++j) a[j].x = a_xy[2 * j], a[j].y = a_xy[2 * j + 1];
	nB[0] = nB[1] = 0; n_anch[0] = n_anch[1] = 0;

	regs0 = mm_gen_regs(0, hash, qlen_sum, n_u, u, a);                                     /* map.c:379 */
	mm_set_parent(0, mask_level, n_regs0, regs0, sub_diff, 0);                             /* chain_post, map.c:249-258 */
	for (i = 0; i < n_regs0; ++i) pre[2 * i] = regs0[i].parent, pre[2 * i + 1] = regs0[i].as;
	if (n_segs <= 1) mm_select_sub(0, pri_ratio, min_diff, best_n, &n_regs0, regs0);
	else mm_select_sub_multi(0, pri_ratio, 0.2f, 0.7f, max_gap_ref, min_diff, best_n, n_segs, qlens, &n_regs0, regs0);
	*nA = n_regs0;
	for (i = 0; i < n_regs0; ++i) put(A + (size_t)i * HITREF_NF, &regs0[i]);

	if (n_segs == 1) {                                                                      /* map.c:390-393 */
		nB[0] = n_regs0;
		n_anch[0] = mate(n_regs0, regs0, a, min_chain_sc, match_sc, rep_len, B, C, anch);
		free(regs0);
	} else {                                                                                /* map.c:394-403 */
		mm_seg_t *seg = mm_seg_gen(0, hash, n_segs, qlens, n_regs0, regs0, n_regs, regs, a);
		int64_t k = 0;
		free(regs0);
		for (s = 0; s < n_segs; ++s) {
			mm_set_parent(0, mask_level, n_regs[s], regs[s], sub_diff, 0);
			nB[s] = n_regs[s];
			n_anch[s] = mate(n_regs[s], regs[s], seg[s].a, min_chain_sc, match_sc, rep_len, B + (size_t)s * n_u * HITREF_NF, C + (size_t)s * n_u * HITREF_NF, anch + 2 * k);
			k += n_anch[s];
			free(regs[s]);
		}
		mm_seg_free(0, n_segs, seg);
	}
	free(u); free(a);
	return 0;
}

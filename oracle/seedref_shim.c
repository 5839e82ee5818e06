/* TEST INFRASTRUCTURE ONLY -- the reference's sketch and seed collection, callable read by read and fragment by fragment
 * (oracle/_ref/libseedref.so, see oracle/Makefile).
 *
 * This file is OUR code and holds none of the reference's.  collect_minimizers() and collect_seed_hits_heap() are static in
 * the fork's map.c, so the Makefile compiles this file with -I$(REF) and the line below pulls map.c in where it lies; the
 * rest of the fork is linked in from its own sources.  Options are mm_set_opt("sr") as oracle/ref_driver.c sets them
 * (MM_F_HEAP_SORT on, no dust filter); k, w and the occurrence bound are the caller's.
 */
#include "map.c"

typedef struct { mm_idx_t *mi; mm_mapopt_t mo; } seedref_t;

seedref_t *seedref_index(int k, int w, int n, const char **seqs, const char **names)
{
	mm_idxopt_t io;
	seedref_t *r = (seedref_t*)calloc(1, sizeof(seedref_t));
	mm_set_opt(0, &io, &r->mo);
	if (mm_set_opt("sr", &io, &r->mo) < 0) { free(r); return 0; }
	r->mi = mm_idx_str(w, k, 0, io.bucket_bits, n, seqs, names);
	if (r->mi == 0) { free(r); return 0; }
	return r;
}

void seedref_destroy(seedref_t *r) { if (r) { mm_idx_destroy(r->mi); free(r); } }

int seedref_flag_ok(const seedref_t *r) { return (r->mo.flag & MM_F_HEAP_SORT) != 0 && r->mo.sdust_thres <= 0; }

/* occurrence list of one minimizer hash (mm_idx_get): its length, and up to cap entries */
int seedref_get(const seedref_t *r, uint64_t minier, uint64_t *out, int cap)
{
	int n = 0, i; const uint64_t *cr = mm_idx_get(r->mi, minier, &n);
	for (i = 0; i < n && i < cap; ++i) out[i] = cr[i];
	return n;
}

/* mm_sketch of one read: the count; up to cap (x, y) pairs into xy */
int64_t seedref_sketch(const char *seq, int len, int w, int k, uint32_t rid, uint64_t *xy, int64_t cap)
{
	mm128_v mv = {0, 0, 0}; int64_t i, n;
	if (len <= 0) return 0;                          /* (mm_sketch asserts len > 0; its callers never hand it an empty read) */
	mm_sketch(0, seq, len, w, k, rid, 0, &mv);
	n = (int64_t)mv.n;
	for (i = 0; i < n && i < cap; ++i) xy[2 * i] = mv.a[i].x, xy[2 * i + 1] = mv.a[i].y;
	free(mv.a);
	return n;
}

/* fragment in, anchors out: n_a (up to cap (x, y) pairs into xy), rep_len, the list count n_m with up to list_cap list lengths, and the minimizer count */
int64_t seedref_frag(const seedref_t *r, int n_segs, const int *qlens, const char **seqs, int max_occ, uint64_t *xy, int64_t cap, int *rep_len, int *n_m, int *n_mv, uint32_t *list_n, int list_cap)
{
	mm128_v mv = {0, 0, 0}; mm128_t *a; mm_match_t *m; uint64_t *mini_pos = 0;
	int i, qlen_sum = 0, n_mini_pos = 0, rep2 = 0; int64_t n_a = 0, n_a2 = 0, j;
	for (i = 0; i < n_segs; ++i) qlen_sum += qlens[i];
	collect_minimizers(0, &r->mo, r->mi, n_segs, qlens, seqs, &mv);
	m = collect_matches(0, n_m, max_occ, r->mi, &mv, &n_a2, &rep2, &n_mini_pos, &mini_pos);
	for (i = 0; i < *n_m && i < list_cap; ++i) list_n[i] = m[i].n;
	kfree(0, m); kfree(0, mini_pos);
	a = collect_seed_hits_heap(0, &r->mo, max_occ, r->mi, 0, &mv, qlen_sum, &n_a, rep_len, &n_mini_pos, &mini_pos);
	for (j = 0; j < n_a && j < cap; ++j) xy[2 * j] = a[j].x, xy[2 * j + 1] = a[j].y;
	*n_mv = (int)mv.n;
	kfree(0, a); kfree(0, mini_pos); kfree(0, mv.a);
	return n_a;
}

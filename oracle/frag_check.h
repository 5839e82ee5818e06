/* TEST INFRASTRUCTURE ONLY -- what alignref_frag() (oracle/alignref_shim.c) and o_frag_align() (oracle/al_oracle.c) require of the caller's chains
 * before they hand them to code that asserts it: chains in the form mm_chain_dp leaves them (one contig and strand per chain, reference and query
 * positions ascending, at least one anchor), every anchor's k-mer inside its contig and inside one mate, spans of at least 1.  OUR code.
 * Returns 0, or the negative number of the rule that failed. */
#ifndef AL_FRAG_CHECK_H
#define AL_FRAG_CHECK_H
#include <stdint.h>

static int frag_check(int n_u, const uint64_t *u, const uint64_t *a_xy, int64_t n_a, int n_segs, const int *qlens, uint32_t n_seq, const uint32_t *seq_len)
{
	int i, s; int64_t k = 0, j, qsum = 0;
	if (n_segs < 1 || n_segs > 2 || n_u < 0 || n_a < 0) return -1;
	for (s = 0; s < n_segs; ++s) { if (qlens[s] < 1) return -2; qsum += qlens[s]; }
	for (i = 0; i < n_u; ++i) {
		const int64_t cnt = (uint32_t)u[i];
		if (cnt < 1 || k + cnt > n_a || (int32_t)(u[i] >> 32) < 1) return -3;
		for (j = k; j < k + cnt; ++j) {
			const uint64_t x = a_xy[2 * j], y = a_xy[2 * j + 1];
			const int64_t rid = (int64_t)(x << 1 >> 33), pos = (int32_t)x, span = (int64_t)(y >> 32 & 0xff), q = (int32_t)y, sid = (int64_t)(y >> 48 & 0xff);
			int64_t acc, q1;
			if (rid >= (int64_t)n_seq || span < 1 || (y >> 56) != 0 || sid >= n_segs) return -4;
			if (pos < 0 || pos + 1 - span < 0 || pos >= (int64_t)seq_len[rid]) return -5;                     /* the k-mer inside its contig */
			acc = sid? qlens[0] : 0;
			q1 = q - ((x >> 63)? qsum - (qlens[sid] + acc) : acc);                                            /* the position inside its mate (hit.c:397) */
			if (q1 + 1 - span < 0 || q1 >= qlens[sid]) return -6;                                             /* ... and inside one mate */
			if (j > k) {
				const uint64_t px = a_xy[2 * (j - 1)], py = a_xy[2 * (j - 1) + 1];
				if ((px >> 32) != (x >> 32)) return -7;                                                         /* one contig, one strand */
				if ((int32_t)px >= (int32_t)x || (int32_t)py >= (int32_t)y) return -8;                          /* ascending on both axes */
			}
		}
		k += cnt;
	}
	return k == n_a? 0 : -10;
}
#endif

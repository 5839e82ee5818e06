// al_kernels_tags.hip -- the MD:Z / cs:Z tags of the fork's --MD and --cs options (write_MD_core / write_cs_core, format.c:137-214),
// computed on the device for every record of a batch after k_compact (and the =/X CIGARs of --eqx before them), so that every output path (device SAM frames, host SAM and BAM
// writers) only splices bytes.  Runs only when AL_F_OUT_MD, AL_F_OUT_CS or AL_F_EQX is set; without them nothing here is launched.
//
// Shape: a 16-lane group per read, records of the read one after the other.  A match run is compared 16 bases per step, lane j on
// base j: reference codes from the index's S4 words, query codes from rd_seq (the packed words the DP reads, in mapping orientation;
// the aligned query is rd_seq[qs, qe), reverse-complemented on the reverse strand -- what format.c:226-234 builds from the original read).
// The group ballot gives the step's mismatch mask; every lane derives the bytes of its own event (run length digits, base letters)
// from the mask and the run carried in from the previous step, and an in-group prefix sum gives its write offset.  k_tag<.., false>
// does the walk counting, k_tag<.., true> repeats it writing into the arena at the record's offset (exclusive scan of the lengths in
// between), so the arena is sized exactly.
#include <hip/hip_runtime.h>
#include <string.h>
#include <cstring>
#include <stdio.h>
#include "al_internal.h"
#include "al_device.h"
#include "al_runtime.h"
#include "al_prim.h"

#define TG 16                              // lanes per read

struct TagIn {
	const AlReg *out; const uint64_t *out_off; const uint32_t *arena;   // records per read (k_compact), CIGAR arena
	const uint32_t *rd_seq; const uint64_t *rd_off;                    // packed reads, mapping orientation
	const uint32_t *S4; const uint64_t *seq_off;                       // reference, 4 bit/base
	uint32_t n_reads;
};

__device__ __forceinline__ int tg_num_len(uint32_t v) { int l = 1; while (v >= 10) { v /= 10; ++l; } return l; }
__device__ __forceinline__ void tg_put_num(char *p, uint32_t v, int l) { char *e = p + l; do { *--e = (char)('0' + v % 10); v /= 10; } while (v); }
__device__ __forceinline__ uint32_t tg_code(const uint32_t *w, uint64_t i) { return (w[i >> 3] >> ((i & 7) << 2)) & 0xfu; }

// in-group inclusive prefix sum (all 16 lanes of the group take part)
__device__ __forceinline__ uint32_t tg_scan(uint32_t v, int lane)
{
#pragma unroll
	for (int d = 1; d < TG; d <<= 1) { const uint32_t u = __shfl_up(v, d, TG); if (lane >= d) v += u; }
	return v;
}

// MODE 0: MD, 1: cs short (":len"), 2: cs long ("=BASES").  WRITE false: byte count per record into len[]; true: bytes into tag[off[k] ..).
template <int MODE, bool WRITE>
__global__ void __launch_bounds__(256)
k_tag(TagIn I, uint32_t *__restrict__ len, const uint64_t *__restrict__ off, char *__restrict__ tag)
{
	const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) / TG; const int lane = threadIdx.x & (TG - 1);
	const int gshift = threadIdx.x & 63 & ~(TG - 1);                   // this group's bits in the wavefront's ballot
	if (i >= I.n_reads) return;
	const uint64_t k0 = I.out_off[i], k1 = I.out_off[i + 1];
	const uint32_t *rd = I.rd_seq + I.rd_off[i];
	for (uint64_t k = k0; k < k1; ++k) {
		const AlReg &r = I.out[k];
		const uint32_t n_cig = (r.flags & ALR_HAS_P) ? r.n_cigar : 0u;
		if (n_cig == 0) { if (!WRITE && lane == 0) len[k] = 0; continue; }
		const uint32_t *cig = r.cigar_off == AL_CIG_INLINE ? r.cig_inl : I.arena + r.cigar_off;
		const bool rev = (r.flags & ALR_REV) != 0;
		const uint64_t tb = I.seq_off[r.rid] + (uint64_t)r.rs;
		char *p = WRITE ? tag + off[k] : nullptr;
		uint32_t n = 0, run = 0;                                       // bytes so far; identity run before the next event (MD: across operations)
		int q_off = 0, t_off = 0;
		for (uint32_t c = 0; c < n_cig; ++c) {
			const int op = cig[c] & 0xf, ol = (int)(cig[c] >> 4);
			if (op == 0 || op == 7 || op == 8) {
				for (int j0 = 0; j0 < ol; j0 += TG) {
					const int j = j0 + lane, cnt = ol - j0 < TG ? ol - j0 : TG;
					const bool act = j < ol;
					uint32_t qc = 4, tc = 4;
					if (act) {
						const int qi = q_off + j;
						qc = rev ? tg_code(rd, (uint64_t)(r.qe - 1 - qi)) : tg_code(rd, (uint64_t)(r.qs + qi));
						if (rev) qc = qc < 4 ? 3 - qc : 4;
						tc = tg_code(I.S4, tb + (uint64_t)(t_off + j));
					}
					const bool mm = act && qc != tc;
					const uint32_t mask = (uint32_t)(__ballot(mm) >> gshift) & 0xffffu;
					const uint32_t below = mask & ((1u << lane) - 1u);
					const uint32_t r_run = below ? (uint32_t)(lane - (31 - __clz(below)) - 1) : run + (uint32_t)lane;   // identity bases right before this lane
					uint32_t b = 0;
					if (MODE == 0) { if (mm) b = tg_num_len(r_run) + 1; }
					else if (MODE == 1) { if (mm) b = 3 + (r_run ? 1 + tg_num_len(r_run) : 0); }
					else { if (mm) b = 3; else if (act) b = 1 + (r_run == 0 ? 1 : 0); }
					const uint32_t incl = tg_scan(b, lane), tot = __shfl(incl, TG - 1, TG);
					if (WRITE && b) {
						char *o = p + n + (incl - b);
						if (MODE == 0) { const int l = (int)b - 1; tg_put_num(o, r_run, l); o[l] = "ACGTN"[tc]; }
						else if (MODE == 1) {
							if (r_run) { const int l = (int)b - 4; o[0] = ':'; tg_put_num(o + 1, r_run, l); o += l + 1; }
							o[0] = '*'; o[1] = "acgtn"[tc]; o[2] = "acgtn"[qc];
						} else if (mm) { o[0] = '*'; o[1] = "acgtn"[tc]; o[2] = "acgtn"[qc]; }
						else { if (b == 2) *o++ = '='; o[0] = "ACGTN"[qc]; }
					}
					n += tot;
					run = mask ? (uint32_t)(cnt - 1 - (31 - __clz(mask))) : run + (uint32_t)cnt;
				}
				q_off += ol; t_off += ol;
				if (MODE == 1 && run) { const int l = tg_num_len(run); if (WRITE && lane == 0) { p[n] = ':'; tg_put_num(p + n + 1, run, l); } n += 1 + l; }
				if (MODE != 0) run = 0;                                // (cs: a run ends with its operation)
			} else if (op == 1) {                                      // insertion: cs "+bases"; MD nothing
				if (MODE != 0) {
					if (WRITE) {
						if (lane == 0) p[n] = '+';
						for (int j = lane; j < ol; j += TG) {
							const int qi = q_off + j;
							uint32_t qc = rev ? tg_code(rd, (uint64_t)(r.qe - 1 - qi)) : tg_code(rd, (uint64_t)(r.qs + qi));
							if (rev) qc = qc < 4 ? 3 - qc : 4;
							p[n + 1 + j] = "acgtn"[qc];
						}
					}
					n += 1 + ol;
				}
				q_off += ol;
			} else if (op == 2) {                                      // deletion: MD "<run>^BASES", cs "-bases"
				const int l = MODE == 0 ? tg_num_len(run) : 0;
				if (WRITE) {
					if (lane == 0) { if (MODE == 0) { tg_put_num(p + n, run, l); p[n + l] = '^'; } else p[n] = '-'; }
					for (int j = lane; j < ol; j += TG) p[n + l + 1 + j] = (MODE == 0 ? "ACGTN" : "acgtn")[tg_code(I.S4, tb + (uint64_t)(t_off + j))];
				}
				n += l + 1 + ol; run = 0;
				t_off += ol;
			} else if (op == 3) t_off += ol;                           // (reference skip: not produced on this path)
		}
		if (MODE == 0 && run) { const int l = tg_num_len(run); if (WRITE && lane == 0) tg_put_num(p + n, run, l); n += l; }
		if (!WRITE && lane == 0) len[k] = n;
	}
}

// --eqx (mm_update_cigar_eqx, align.c:169-238): every M operation split into maximal = / X runs (N against N is =).  Same group walk:
// the boundaries of a 16-base step are where the mismatch bit changes (or the operation starts); each boundary but an operation's
// first closes the run before it, and that lane writes the closed run's word; the run still open at the operation's end is written
// by lane 0.  WRITE false: words per record into cnt[]; true: the words into cig[off[k] ..).
template <bool WRITE>
__global__ void __launch_bounds__(256)
k_eqx(TagIn I, uint32_t *__restrict__ cnt, const uint64_t *__restrict__ off, uint32_t *__restrict__ cig_out)
{
	const uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) / TG; const int lane = threadIdx.x & (TG - 1);
	const int gshift = threadIdx.x & 63 & ~(TG - 1);
	if (i >= I.n_reads) return;
	const uint64_t k0 = I.out_off[i], k1 = I.out_off[i + 1];
	const uint32_t *rd = I.rd_seq + I.rd_off[i];
	for (uint64_t k = k0; k < k1; ++k) {
		const AlReg &r = I.out[k];
		const uint32_t n_cig = (r.flags & ALR_HAS_P) ? r.n_cigar : 0u;
		if (n_cig == 0) { if (!WRITE && lane == 0) cnt[k] = 0; continue; }
		const uint32_t *cig = r.cigar_off == AL_CIG_INLINE ? r.cig_inl : I.arena + r.cigar_off;
		const bool rev = (r.flags & ALR_REV) != 0;
		const uint64_t tb = I.seq_off[r.rid] + (uint64_t)r.rs;
		uint32_t *o = WRITE ? cig_out + off[k] : nullptr;
		uint32_t n = 0; int q_off = 0, t_off = 0;
		for (uint32_t c = 0; c < n_cig; ++c) {
			const uint32_t w = cig[c]; const int op = w & 0xf, ol = (int)(w >> 4);
			if (op != 0) {
				if (WRITE && lane == 0) o[n] = w;
				++n;
				if (op == 1 || op == 4 || op == 7 || op == 8) q_off += ol;
				if (op == 2 || op == 3 || op == 7 || op == 8) t_off += ol;
				continue;
			}
			uint32_t pc = 0; int start = 0;                            // class of the last base of the previous step; start of the open run
			for (int j0 = 0; j0 < ol; j0 += TG) {
				const int j = j0 + lane, cn = ol - j0 < TG ? ol - j0 : TG;
				uint32_t qc = 4, tc = 4;
				if (j < ol) {
					const int qi = q_off + j;
					qc = rev ? tg_code(rd, (uint64_t)(r.qe - 1 - qi)) : tg_code(rd, (uint64_t)(r.qs + qi));
					if (rev) qc = qc < 4 ? 3 - qc : 4;
					tc = tg_code(I.S4, tb + (uint64_t)(t_off + j));
				}
				const uint32_t am = cn == TG ? 0xffffu : (1u << cn) - 1u;
				const uint32_t mask = (uint32_t)(__ballot(j < ol && qc != tc) >> gshift) & am;
				const uint32_t B = (mask ^ ((mask << 1) | pc)) & am;       // boundaries of this step
				const uint32_t E = j0 == 0 ? B & ~1u : B;                 // ... that close a run
				if (WRITE && ((E >> lane) & 1u)) {
					const uint32_t lb = B & ((1u << lane) - 1u);
					const int s0 = lb ? j0 + (31 - __clz(lb)) : start;
					const uint32_t cls = lane ? (mask >> (lane - 1)) & 1u : pc;
					o[n + __popc(E & ((1u << lane) - 1u))] = (uint32_t)(j - s0) << 4 | (cls ? 8u : 7u);
				}
				n += __popc(E);
				if (B) start = j0 + (31 - __clz(B));
				pc = (mask >> (cn - 1)) & 1u;
			}
			if (WRITE && lane == 0) o[n] = (uint32_t)(ol - start) << 4 | (pc ? 8u : 7u);
			++n;
			q_off += ol; t_off += ol;
		}
		if (!WRITE && lane == 0) cnt[k] = n;
	}
}
// the records take their =/X CIGARs: four operations or fewer inline (AL_CIG_INLINE), longer ones at their place in the new arena
__global__ void __launch_bounds__(256)
k_eqx_fix(AlReg *__restrict__ out, uint64_t n_out, const uint32_t *__restrict__ cnt, const uint64_t *__restrict__ off, const uint32_t *__restrict__ cig)
{
	const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= n_out) return;
	AlReg &r = out[k];
	if (!(r.flags & ALR_HAS_P) || r.n_cigar == 0) return;
	const uint32_t n = cnt[k];
	r.n_cigar = n;
	if (n <= 4) { for (uint32_t j = 0; j < n; ++j) r.cig_inl[j] = cig[off[k] + j]; r.cigar_off = AL_CIG_INLINE; }
	else r.cigar_off = (uint32_t)off[k];
}

template <int MODE>
static void launch_tag(const TagIn &I, bool write, uint32_t *len, const uint64_t *off, char *tag, hipStream_t s)
{
	const dim3 g((unsigned)(((uint64_t)I.n_reads * TG + 255) / 256)), b(256);
	if (write) hipLaunchKernelGGL((k_tag<MODE, true>), g, b, 0, s, I, len, off, tag);
	else hipLaunchKernelGGL((k_tag<MODE, false>), g, b, 0, s, I, len, off, tag);
}

int al_run_eqx_stage(al_ctx_t *c, AlReg *out, const uint64_t *out_off, uint64_t n_out, const uint32_t *arena, AlTagBufs &E)
{
	hipStream_t s = c->stream;
	E.bytes = 0;
	if (E.len.ensure(n_out + 1) || E.off.ensure(n_out + 1)) return -1;
	AL_HIP_CHECK(hipMemsetAsync(E.len.p + n_out, 0, 4, s));
	TagIn I{out, out_off, arena, c->rd_seq.p, c->rd_off.p, c->di.S4, c->di.seq_off, (uint32_t)c->n_reads};
	const dim3 g((unsigned)(((uint64_t)I.n_reads * TG + 255) / 256)), b(256);
	if (I.n_reads) hipLaunchKernelGGL((k_eqx<false>), g, b, 0, s, I, E.len.p, (const uint64_t *)nullptr, (uint32_t *)nullptr);
	if (al_prim_scan_u32_u64(c->scan_tmp, E.len.p, E.off.p, (size_t)n_out + 1, s)) return -1;
	uint64_t words = 0;
	AL_HIP_CHECK(hipMemcpyAsync(&words, E.off.p + n_out, 8, hipMemcpyDeviceToHost, s));
	AL_HIP_CHECK(hipStreamSynchronize(s));
	if (words >= 0xfffffff0ULL) { fprintf(stderr, "[airlift] =/X CIGARs of one batch exceed the 32-bit arena index\n"); al_nomem_flag() = true; return -1; }
	if (E.arena.ensure((words + 4) * 4)) return -1;
	uint32_t *cw = (uint32_t *)E.arena.p;
	if (I.n_reads && words) hipLaunchKernelGGL((k_eqx<true>), g, b, 0, s, I, E.len.p, (const uint64_t *)E.off.p, cw);
	if (n_out) hipLaunchKernelGGL(k_eqx_fix, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, out, n_out, (const uint32_t *)E.len.p, (const uint64_t *)E.off.p, (const uint32_t *)cw);
	AL_HIP_CHECK(hipGetLastError());
	AL_HIP_CHECK(hipStreamSynchronize(s));                             // the host drivers copy records and arena with plain hipMemcpy
	E.bytes = words;
	return 0;
}

int al_run_tag_stage(al_ctx_t *c, const AlReg *out, const uint64_t *out_off, uint64_t n_out, const uint32_t *arena, AlTagBufs &T)
{
	hipStream_t s = c->stream;
	const int64_t fl = c->opt.flag;
	const int mode = (fl & AL_F_OUT_MD) ? 0 : (fl & AL_F_OUT_CS_LONG) ? 2 : 1;   // MD wins over cs (format.c:533: is_MD)
	T.bytes = 0;
	if (T.len.ensure(n_out + 1) || T.off.ensure(n_out + 1)) return -1;
	AL_HIP_CHECK(hipMemsetAsync(T.len.p + n_out, 0, 4, s));
	TagIn I{out, out_off, arena, c->rd_seq.p, c->rd_off.p, c->di.S4, c->di.seq_off, (uint32_t)c->n_reads};
	if (I.n_reads) {
		if (mode == 0) launch_tag<0>(I, false, T.len.p, nullptr, nullptr, s);
		else if (mode == 1) launch_tag<1>(I, false, T.len.p, nullptr, nullptr, s);
		else launch_tag<2>(I, false, T.len.p, nullptr, nullptr, s);
	}
	if (al_prim_scan_u32_u64(c->scan_tmp, T.len.p, T.off.p, (size_t)n_out + 1, s)) return -1;
	uint64_t bytes = 0;
	AL_HIP_CHECK(hipMemcpyAsync(&bytes, T.off.p + n_out, 8, hipMemcpyDeviceToHost, s));
	AL_HIP_CHECK(hipStreamSynchronize(s));
	if (bytes >= (1ULL << 32)) { fprintf(stderr, "[airlift] tags of one batch exceed 4 GB\n"); al_nomem_flag() = true; return -1; }   // (the SAM frames address the arena with 32 bits: a smaller batch)
	if (T.arena.ensure(bytes + 16)) return -1;
	if (I.n_reads && bytes) {
		if (mode == 0) launch_tag<0>(I, true, T.len.p, T.off.p, T.arena.p, s);
		else if (mode == 1) launch_tag<1>(I, true, T.len.p, T.off.p, T.arena.p, s);
		else launch_tag<2>(I, true, T.len.p, T.off.p, T.arena.p, s);
	}
	AL_HIP_CHECK(hipGetLastError());
	AL_HIP_CHECK(hipStreamSynchronize(s));                             // the host drivers copy the arena with plain hipMemcpy (not ordered behind this stream)
	T.bytes = bytes;
	return 0;
}

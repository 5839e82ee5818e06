/* airlift.h -- C-ABI of the MI355X-native AirLift re-alignment path (libairlift.so).
 *
 * Drop-in boundary for the one hot path AirLift delegates to an external aligner:
 *   src/0-align_reads.sh:13, src/0-align_singletons.sh:12, src/3-align_gaps/align_gaps.sh:14-15
 * (process level: `airlift-align` CLI), and, at library level, the C API of the bundled
 * minimap2 fork (src/minimap2-master_remapping/minimap.h) for the `-ax sr` path.  Each entry point
 * below names the reference declaration it replaces.  Plain pointers and sizes only.
 *
 * Ownership / threading rules are the reference's (minimap.h:296-331): the index is immutable and
 * shareable after build; one al_ctx_t per host thread (it owns a HIP stream and device workspaces);
 * hit arrays returned by al_map_frag() and each al_reg1_t::cigar are malloc()ed by the callee and
 * free()d by the caller.  Errors: NULL / negative return, message on stderr; there is NO CPU
 * fallback -- without a usable HIP device al_ctx_init() fails loudly.
 */
#ifndef AIRLIFT_H
#define AIRLIFT_H

#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AL_VERSION "0.1.0"

/* flag bits: same values as MM_F_* (minimap.h:8-38) for the subset this path uses */
#define AL_F_CIGAR         0x004
#define AL_F_OUT_SAM       0x008
#define AL_F_SR            0x1000
#define AL_F_FRAG_MODE     0x2000
#define AL_F_NO_PRINT_2ND  0x4000
#define AL_F_HEAP_SORT     0x400000
#define AL_F_SAM_HIT_ONLY  0x40000000
/* output options (main.c:164, 207, 210, 223-233): cs:Z / MD:Z tags, soft clips and full SEQ on supplementaries (-Y), =/X CIGARs (--eqx; also what al_map_frag returns) */
#define AL_F_OUT_CS        0x40
#define AL_F_OUT_CS_LONG   0x800
#define AL_F_SOFTCLIP      0x80000
#define AL_F_OUT_MD        0x1000000
#define AL_F_EQX           0x4000000
/* PAF output (main.c:158, 211; format.c:304-330).  The fork writes PAF whenever MM_F_OUT_SAM is clear; here callers of al_set_opt never set
 * AL_F_OUT_SAM and get SAM, so PAF has a flag of its own above the fork's 32 bits.  Only under AL_F_OUT_PAF is AL_F_CIGAR looked at: clear = no
 * base-level alignment (the fork's `-x sr` without -a / -c, map.c:262, 404): chaining, per-mate hits and MAPQ only; records carry n_cigar == 0. */
#define AL_F_OUT_CG        0x020            /* -c: cg:Z: CIGAR in PAF */
#define AL_F_PAF_NO_HIT    0x8000000        /* --paf-no-hit: a `name len 0 0 * * 0 0 0 0 0 0` line for a read without hits */
#define AL_F_OUT_PAF       0x100000000LL    /* --paf (no analogue in the fork: its default) */
/* Input: BGZF-compressed FASTQ files (bgzip, bcl-convert, DRAGEN) of the file-mapping calls stay with the stream driver, their members inflated on the
 * GPU straight into the batch text.  Decided per file; without the flag, or for a gzip file that is not BGZF, the host reader inflates as before. */
#define AL_F_IN_GPU_INFLATE 0x200000000LL   /* --gpu-inflate of the mapping commands (no analogue in the fork) */

/* replaces mm_idxopt_t (minimap.h:101-105) */
typedef struct {
	short k, w, flag, bucket_bits;
	int mini_batch_size;
	uint64_t batch_size;
} al_idxopt_t;

/* replaces mm_mapopt_t (minimap.h:107-152); same field names and meaning */
typedef struct {
	int64_t flag;
	int seed;
	int bw;
	int max_gap, max_gap_ref;
	int max_frag_len;
	int max_chain_skip, max_chain_iter;
	int min_cnt;
	int min_chain_score;
	float mask_level;
	float pri_ratio;
	int best_n;
	int a, b, q, e, q2, e2;
	int sc_ambi;
	int zdrop, zdrop_inv;
	int end_bonus;
	int min_dp_max;
	float max_clip_ratio;
	int pe_ori, pe_bonus;
	int32_t mid_occ;
	int32_t max_occ;
	int mini_batch_size;
} al_mapopt_t;

/* replaces mm_reg1_t + mm_extra_t (minimap.h:74-98) */
typedef struct {
	int32_t id, cnt, rid, score;
	int32_t qs, qe, rs, re;
	int32_t parent, subsc;
	int32_t mlen, blen;
	int32_t n_sub, score0;
	uint32_t mapq:8, split:2, rev:1, inv:1, sam_pri:1, proper_frag:1, pe_thru:1, seg_split:1, seg_id:8, split_inv:1, dummy:7;
	uint32_t hash;
	int32_t dp_score, dp_max, dp_max2;
	uint32_t n_ambi;
	uint32_t n_cigar;
	uint32_t *cigar;             /* BAM-encoded, malloc()ed; NULL if n_cigar == 0 */
} al_reg1_t;

typedef struct al_idx_s al_idx_t;   /* replaces mm_idx_t (minimap.h:63-72); opaque, own HBM-oriented layout */
typedef struct al_ctx_s al_ctx_t;   /* replaces mm_tbuf_t (minimap.h:296-310): per-thread buffer = HIP stream + workspaces */

/* mm_set_opt (minimap.h:180): preset NULL = defaults; "sr"/"short" = AirLift's preset; else -1 */
int  al_set_opt(const char *preset, al_idxopt_t *io, al_mapopt_t *mo);
/* mm_check_opt (minimap.h:181): 0 if usable on this path, negative otherwise (message on stderr) */
int  al_check_opt(const al_idxopt_t *io, const al_mapopt_t *mo);

/* mm_idx_reader_open + mm_idx_reader_read (minimap.h:206-232) for a FASTA(.gz) file: NULL on failure */
al_idx_t *al_idx_build(const char *fn, const al_idxopt_t *io, int n_threads);
/* Same index, built on the GPU (sketch, sort and table construction as kernels; the host only parses the FASTA): the
 * index stays resident on `device` (< 0: LOCAL_RANK or 0) and is copied device-to-device if a context on another GPU
 * asks for it.  Needs odd k.  NULL (with a message) if HIP is unusable -- there is no host path behind this entry point. */
al_idx_t *al_idx_build_device(const char *fn, const al_idxopt_t *io, int device);
/* mm_idx_reader_open / mm_idx_reader_read / mm_idx_reader_eof / mm_idx_reader_close (minimap.h:206-232): the reference's
 * iterator over index parts.  This path builds one part: the first read() returns the whole index (built on `device`, as
 * al_idx_build_device), the next NULL.  A file that starts with the index magic (mm_idx_is_idx, index.c:531) is a prebuilt index and is loaded instead; fn_out
 * (minimap2's -d) makes read() write the index it built there.  open() returns NULL if the file cannot be opened. */
typedef struct al_idx_reader_s al_idx_reader_t;
al_idx_reader_t *al_idx_reader_open(const char *fn, const al_idxopt_t *io, const char *fn_out);
al_idx_t *al_idx_reader_read(al_idx_reader_t *r, int device);
int       al_idx_reader_eof(const al_idx_reader_t *r);
void      al_idx_reader_close(al_idx_reader_t *r);
/* mm_idx_dump / mm_idx_load / mm_idx_is_idx (index.c:438-552): the reference's index file, both ways -- an .mmi the fork wrote is read here, one written here is read
 * by the fork (the files differ in the order of a bucket's hash pairs only).  dump copies a device-built index off the GPU first; 0 / -1. */
int       al_idx_dump(const char *fn, al_idx_t *mi);
al_idx_t *al_idx_load(const char *fn);
int64_t   al_idx_is_idx(const char *fn);
int       al_idx_k(const al_idx_t *mi);      /* mm_idx_t::k, ::w (minimap.h:57) */
int       al_idx_w(const al_idx_t *mi);
/* Batch API: the caller will not read the sorted-anchor taps (al_dbg_anchors after a run) of this context, so the alignment stage's per-mate anchor arrays take the
 * place of their copy: 16 bytes per seed hit less (20 GB on a 1 M-pair batch against a human-sized reference).  The file drivers set it for their contexts. */
void      al_ctx_set_no_taps(al_ctx_t *ctx, int on);
/* mm_idx_cal_max_occ (index.c:164-185): (1-f) quantile of the per-minimizer occurrence counts + 1; INT32_MAX for f <= 0 */
int32_t   al_idx_cal_max_occ(const al_idx_t *mi, float f);
/* mm_mapopt_update (minimap.h:183, options.c:51-61): mid_occ <= 0 is replaced by al_idx_cal_max_occ(mi, 2e-4) */
void      al_mapopt_update(al_mapopt_t *opt, const al_idx_t *mi);
/* mm_idx_str (minimap.h:269) */
al_idx_t *al_idx_str(int w, int k, int n, const char **seq, const char **name);
/* mm_idx_destroy (minimap.h:291) */
void      al_idx_destroy(al_idx_t *mi);
uint32_t  al_idx_n_seq(const al_idx_t *mi);
const char *al_idx_seq_name(const al_idx_t *mi, uint32_t rid);
uint32_t  al_idx_seq_len(const al_idx_t *mi, uint32_t rid);
/* mm_idx_stat-like numbers: distinct minimizers, total positions, total bases */
void      al_idx_stat(const al_idx_t *mi, uint64_t *n_keys, uint64_t *n_pos, uint64_t *n_bases);
/* the occurrence array (all positions, grouped by minimizer hash ascending, ascending inside a group): returns the
 * number of entries and copies up to cap of them; for tests that compare the two builders */
int64_t   al_idx_export_pos(const al_idx_t *mi, uint64_t *dst, int64_t cap);

/* mm_tbuf_init / mm_tbuf_destroy (minimap.h:303,310).  device < 0: use LOCAL_RANK or 0.
 * Uploads the index to that device's HBM on first use.  NULL (with a message) if HIP is unusable. */
al_ctx_t *al_ctx_init(const al_idx_t *mi, const al_mapopt_t *opt, int device);
void      al_ctx_destroy(al_ctx_t *ctx);
/* host worker threads this context may use for packing a batch before upload (default 1); the analogue of the
 * n_threads argument of mm_map_file_frag for callers that drive batches themselves */
void      al_ctx_set_threads(al_ctx_t *ctx, int n_threads);

/* mm_map_frag (minimap.h:334): one fragment of n_segs (1 or 2) reads, reads given in sequencing
 * orientation; output identical in meaning to the reference incl. the FR flip of worker_for (map.c:458-498). */
void al_map_frag(const al_idx_t *mi, int n_segs, const int *qlens, const char **seqs, int *n_regs,
                 al_reg1_t **regs, al_ctx_t *ctx, const al_mapopt_t *opt, const char *qname);

/* Batch entry point (no reference analogue; the reference's kt_for over fragments, map.c:592).
 * reads are listed fragment-major: n_segs[f] reads for fragment f.  On return n_regs[i] / regs[i]
 * (i over reads) are filled like al_map_frag; rep_len[f] gets the fragment's repeat length.
 * Returns 0, or negative on error. */
int  al_map_batch(al_ctx_t *ctx, int n_frag, const int *n_segs, const int *qlens, const char *const *seqs,
                  const char *const *qnames, int *n_regs, al_reg1_t **regs, int *rep_len);

/* mm_map_file_frag (minimap.h:348): map 1 or 2 FASTA/FASTQ(.gz) files, SAM to `out` (header included
 * when rg != (char*)-1; pass rg = NULL for no @RG).  Returns 0, -1 if a file cannot be read. */
int  al_map_file_frag(const al_idx_t *mi, int n_segs, const char **fn, const al_mapopt_t *opt, int n_threads,
                      FILE *out, const char *rg, int device);

/* Same mapping, BAM on `out` instead of SAM text (BGZF blocks deflated at `level`, 0-9; n_threads workers).  sorted == 0: input
 * order, the same records as the SAM output.  sorted != 0: mapped records only, coordinate-sorted -- what AirLift produces with
 * `| samtools view -h -F4 | samtools sort -l5` (src/0-align_reads.sh:13, run_pipeline.sh:82-87). */
int  al_map_file_frag_bam(const al_idx_t *mi, int n_segs, const char **fn, const al_mapopt_t *opt, int n_threads,
                          FILE *out, const char *rg, int device, int sorted, int level);
/* OR-ed into `level` of al_map_file_frag_bam: the BGZF blocks are deflated on `device` instead of the host's worker threads (the CLI's
 * --gpu-deflate).  Level 0 stores; every other level selects the one device compressor.  The uncompressed stream and its cut into blocks
 * are those of the host-deflated file; the compressed bytes are a function of each block's bytes alone.  Without the bit nothing changes (a
 * level outside 0-9 means 5).  One device, one process: al_map_file_frag_multi with n_dev > 1 and al_map_file_frag_ranked_bam return -1
 * with a message when the bit is set. */
#define AL_BAM_DEFLATE_DEVICE 0x100

/* Several GPUs of one node (the reference's analogue is kt_for over the fragments of a mini-batch, map.c:592, with
 * its serial ordered writer, map.c:601-644): lane r is a mapping context on devices[r] (a device may appear twice: two lanes
 * overlap transfers and kernels on it); every mini-batch is cut into n_dev contiguous fragment ranges, lane r maps range r.
 * The index is built once and copied device to device.  The lanes exchange only {records, bytes} of their output blocks per
 * batch (a 16-byte ncclAllGather over xGMI when they sit on distinct GPUs), take the exclusive prefix sum as their file offset
 * and pwrite() their block when `out` is a regular file (ordered turns otherwise).  bam_mode 0 SAM, 1 BAM, 2 sorted BAM.
 * Output bytes are those of al_map_file_frag / al_map_file_frag_bam. */
int  al_map_file_frag_multi(const al_idx_t *mi, int n_segs, const char **fn, const al_mapopt_t *opt, int n_threads,
                            FILE *out, const char *rg, const int *devices, int n_dev, int bam_mode, int level);

/* One process per GPU: rank `rank` of `world` maps a contiguous range of the input's fragments -- it finds its own byte
 * ranges of the plain FASTQ files (line counts of every rank's share, exchanged once) -- and writes its SAM text into `out_path` at the
 * offset the final all-gather of {ok, bytes} per rank gives it (rank-major = input order).  The exchanges are 16-byte all-gathers: RCCL
 * over xGMI when every rank has its own GPU, files in `rendezvous` (default: the output's directory) otherwise; a rank that does not
 * arrive within timeout_s (<= 0: AL_RANK_TIMEOUT or 600) makes the others fail.  device < 0: LOCAL_RANK or `rank`.  Output bytes are
 * those of al_map_file_frag on the whole input. */
int  al_map_file_frag_ranked(const al_idx_t *mi, int n_segs, const char **fn, const al_mapopt_t *opt, int n_threads, const char *out_path,
                             const char *rg, int device, int rank, int world, const char *rendezvous, double timeout_s);
/* The same with unsorted BAM output: every rank deflates its own records into whole BGZF blocks (rank 0's part carries the header, the last
 * rank's the EOF block), the parts go behind each other at the exchanged offsets.  Decoded records = those of al_map_file_frag_bam. */
int  al_map_file_frag_ranked_bam(const al_idx_t *mi, int n_segs, const char **fn, const al_mapopt_t *opt, int n_threads, const char *out_path,
                                 const char *rg, int device, int rank, int world, const char *rendezvous, double timeout_s, int bam_level);
/* Self-test of the range finding of al_map_file_frag_ranked without a GPU: `world` threads act as the ranks; 0 = the ranges tile the
 * files, start at records and pair record for record. */
int  al_dbg_ranked_selftest(const char *fn1, const char *fn2, int world, const char *dir);

/* ---- read extraction feeding the path (host-side; replaces per-region `samtools view | convert2bed | awk`) ---- */
/* src/4-extract_reads/extract_reads.sh:8 (prune != 0) / extract_reads_noprune.sh:7 (prune == 0) for all lines of a BED file in
 * one pass over the BAM: rows "chrom start end name[.1|.2] MAPQ CIGAR" of the mapped records that lie inside a BED line
 * (start >= B-1, end <= E-1) and, when pruning, have MAPQ <= 10 or a CIGAR other than "<read_size>M"; one row per name,
 * sorted by name (`sort -uk4,4`).  Returns the number of rows, negative on error. */
int64_t al_extract_reads(const char *bam_fn, const char *bed_fn, int read_size, int prune, FILE *out);
/* The same rows with a choice of reader.  flags & AL_EXTRACT_GPU_INFLATE (the CLI's --gpu-inflate): the BGZF members of the BAM are inflated on
 * `device` (-1: the default device) by k_inflate, a piece of the file at a time, CRC32 checked there; where the device has no memory for the
 * reader's buffers they are inflated by zlib on n_threads host threads instead (one notice on stderr).  A member that does not inflate, a wrong
 * CRC32 and a truncated last member are error -2, with the member's file offset on stderr.  A gzip file that is not BGZF, and "-", are read as one
 * gzip stream, as al_extract_reads does.  flags == 0 is al_extract_reads.  (Test switches: DESIGN.md section 8.) */
#define AL_EXTRACT_GPU_INFLATE 1u
int64_t al_extract_reads_ex(const char *bam_fn, const char *bed_fn, int read_size, int prune, FILE *out, unsigned flags, int device, int n_threads);
/* src/4-extract_reads/extract_sequence.sh:17-19: FASTQ subsets by the names in column 4 of `rows_fn` (seqtk subseq), pairing
 * (BBMap repair.sh) and renaming (rename.sh: realigned_<n>, realigned_singleton_<n>) into out_dir/reads_1.fastq,
 * reads_2.fastq, singletons.fastq.  Returns 0, negative on error. */
int  al_extract_sequence(const char *fq1, const char *fq2, const char *rows_fn, const char *out_dir, int64_t *n_pairs, int64_t *n_single);
/* The same with a choice of selector.  flags & AL_EXTRACT_GPU_SELECT (the CLI's --gpu-select): the FASTQ bytes go to `device` (-1: the default device) as
 * they are, kernels test every record's name against the selected names and only the selected records come back; with AL_EXTRACT_GPU_INFLATE as well, a BGZF
 * FASTQ file is inflated there.  Another gzip file, or "-", takes the default reader, with a notice.  AL_EXTRACT_SELECT_HOST: the same driver with the
 * function evaluated on the host (tests, machines without a GPU); it is also what runs, with a notice, where the device or its memory is refused.
 * piece_bytes: the file piece (0: 8 MB; of a BGZF file 4 x AL_INFLATE_PIECE_KB of text).  n_threads is reserved.  The output is byte for byte that of al_extract_sequence; flags == 0 is that function. */
#define AL_EXTRACT_GPU_SELECT 2u
#define AL_EXTRACT_SELECT_HOST 4u
int  al_extract_sequence_ex(const char *fq1, const char *fq2, const char *rows_fn, const char *out_dir, int64_t *n_pairs, int64_t *n_single,
                            unsigned flags, int device, int n_threads, size_t piece_bytes);
/* N1 fused: extract_reads.sh:8 + extract_sequence.sh:17-19 in one call, nothing written to disk.  The three FASTQ texts
 * (pairs file 1, pairs file 2, singletons) are left in anonymous memory files whose descriptors go to fds[0..2]; map them by path
 * ("/proc/self/fd/<n>") with al_map_file_frag -- `airlift-align remap` does exactly that -- and close() them.  0, negative on error. */
int  al_extract_to_memory(const char *bam_fn, const char *bed_fn, int read_size, int prune, const char *fq1, const char *fq2, int fds[3], int64_t *n_pairs, int64_t *n_single);
/* ... with flags, device, n_threads as al_extract_reads_ex, and AL_EXTRACT_GPU_SELECT / AL_EXTRACT_SELECT_HOST as al_extract_sequence_ex (piece: the default);
 * the reader's and the selector's device and page-locked buffers are released before it returns. */
int  al_extract_to_memory_ex(const char *bam_fn, const char *bed_fn, int read_size, int prune, const char *fq1, const char *fq2, int fds[3], int64_t *n_pairs, int64_t *n_single,
                             unsigned flags, int device, int n_threads);
/* Taps of the BGZF inflater (al_dev_inflate.h, al_inflate.hip; tests).  src[0, n) is a sequence of whole BGZF members: they are listed along the BSIZE
 * chain and inflated to dst (cap bytes), member m at the sum of ISIZE of the members before it; *out_n = that sum over all, status[m] = 0 or the
 * member's error (AL_INF_E_*: 1 header, 2 block type, 3 stored lengths, 4 code lengths, 5 symbol, 6 distance, 7 input exhausted, 8 over ISIZE,
 * 9 short of ISIZE, 10 CRC), *n_members = members listed.  0; -2 when the chain breaks (no BC subfield, BSIZE past the end: the members before are
 * done); -3 when cap or n_status is too small; -1 when a HIP call fails.  _host: the host twin, serially.  The device tap: k_inflate over the whole
 * list in one launch.  _guard: the same with the output between two poisoned ranges of 64 KB, -7 when the kernel wrote into one. */
int  al_dbg_bgzf_inflate_host(const void *src, size_t n, void *dst, size_t cap, size_t *out_n, uint32_t *status, size_t n_status, size_t *n_members);
int  al_dbg_bgzf_inflate(int device, const void *src, size_t n, void *dst, size_t cap, size_t *out_n, uint32_t *status, size_t n_status, size_t *n_members);
int  al_dbg_bgzf_inflate_guard(int device, const void *src, size_t n, void *dst, size_t cap, size_t *out_n, uint32_t *status, size_t n_status, size_t *n_members);
/* Test taps of --gpu-select: one text and one list of names (each followed by '\n') through ONE pass of the product's kernels (al_dbg_fq_select) or of
 * their host twin (al_dbg_fq_select_host).  flags[0, *n_rec): 0 / 1 per parsed record (n_flags of room); *first_bad: the first record that is not regular
 * (~0: none); arena[0, *arena_n) and desc (three words per selected record in front of first_bad: arena offset, name length, sequence length; desc_cap
 * records of room, *n_sel used).  0; -1: the device failed; -3: an array is too small (the counts are set). */
int  al_dbg_fq_select_host(const void *text, size_t n, const char *names, size_t names_len, uint32_t *flags, size_t n_flags, uint64_t *n_rec, uint64_t *first_bad,
                           void *arena, size_t arena_cap, size_t *arena_n, uint32_t *desc, size_t desc_cap, size_t *n_sel);
int  al_dbg_fq_select(int device, const void *text, size_t n, const char *names, size_t names_len, uint32_t *flags, size_t n_flags, uint64_t *n_rec, uint64_t *first_bad,
                      void *arena, size_t arena_cap, size_t *arena_n, uint32_t *desc, size_t desc_cap, size_t *n_sel);

/* Tap (parity tests): the extension DP alone -- ksw_extd2_sse's result for n caller-supplied pairs, as the reference's --print-aln-seq
 * shows them (align.c:313-339).  seqs: nt4 codes (0..4); jobs6: {target offset, query offset, tlen, qlen, ksw flag, 0} per pair (the
 * sequences as passed to ksw, i.e. already reversed for left extensions); out9 per pair: score, max, max_q, max_t, mqe, mqe_t, zdropped,
 * reach_end, n_cigar (-1: pair larger than 1024 x 512); cig_out: cig_cap words per pair.  Uses the context's options.
 * Runs the DP's device functions on LDS rows of its own, not the align stage's kernels: the one-cell-per-lane forms (register blocks up to
 * 22 x 16 target bases, LDS rows above), with AL_DBG bit 20 the two-cells-per-lane form on pairs of up to 352 target bases where the
 * align stage would use it too (scores inside that form's arithmetic), without the early exit.  tests/test_gpu_dp_directed.py compares every
 * field with ksw_extd2_sse; the align stage's own kernels are reached through al_dbg_ext_dp. */
int  al_dbg_ksw(al_ctx_t *ctx, int n, const uint8_t *seqs, size_t n_seq_bytes, const int32_t *jobs6, int32_t *out9, uint32_t *cig_out, int cig_cap);
/* Tap (parity tests): n caller-supplied extension jobs through the align stage's DP kernels -- keyed into classes, counted, sorted and launched
 * by the code the stage runs for the jobs of a batch, so which kernel instance a job takes follows from its size, its direction and the list
 * around it exactly as in a batch.  Needs a batch uploaded with al_batch_upload (the queries are read from its reads) and run once.
 * jobs8 per job: read index, rev (1: the read's reverse complement), kind (0 = left extension: query and target are walked downwards from
 * qoff / tpos and the ksw flags are EXTZ_ONLY | RIGHT | REV_CIGAR; 1 = right extension: upwards, EXTZ_ONLY), qoff (into the read as oriented
 * by rev), qlen, contig, tpos (into the contig), tlen.  out9 per job: max, max_q, max_t, mqe_t, reach_end, zdropped, n_cigar, the job's class
 * (0, 1 lane per job with targets <= 16 / 32; 3 ... 8 group DP of 1, 2, 4, 8, 22, 32 target blocks; 9 LDS rows), 1 if the CIGAR did not fit
 * cig_cap words or the kernels' own buffers.  cig_out: cig_cap words per job.  shadow8 (may be NULL): the early exit's shadow counts of this
 * call (AL_DBG2 bit 5): jobs, jobs whose exit-row state differs from the full run's, rows, rows needed, ...  The per-class job counts are left
 * in al_batch_stat's dp_jobs.  Returns 0; -2: a job lies outside its read, its contig or what the stage can emit for this batch (nothing ran);
 * -3: the batch's reads are too long for the stage to run DP jobs at all. */
int  al_dbg_ext_dp(al_ctx_t *ctx, int n, const int64_t *jobs8, int32_t *out9, uint32_t *cig_out, int cig_cap, uint64_t *shadow8);
/* Tap (parity tests): the chain stage on caller-supplied anchors, through the code the stage runs for a batch: the fragments are keyed into
 * size classes and ordered, the small ones go to the lane kernels, the others to the tile kernel or the segment-wise kernels as the options and
 * the environment switches decide, the flagged ones to the second round, and whatever the kernels hand back takes the fallback and the chain-order
 * kernels.  Needs a batch uploaded with al_batch_upload and NOT run: its fragments, read lengths and longest fragment are what the kernels derive
 * max_dist_x / max_dist_y from (dummy reads of the wanted lengths will do).  anchors_xy: (x, y) pairs of all fragments, each fragment's in
 * ascending x; a_off[n_frag + 1]: first anchor of every fragment; tie_flag[n_frag]: 1 = the fragment has anchors of equal x (what the sort kernels
 * flag: chained in the second round).  Out, laid out as the context's arrays: nu_out[n_frag]; u_out / uo_out[a_off[n_frag] + n_frag + 1], the
 * chain list of fragment f from a_off[f] + f on (u = score << 32 | anchors; uo = offset of the chain's anchors in the fragment's range);
 * chained_xy: a_off[n_frag] anchors.  counts[24] (may be NULL): fragments the lane kernels took up to 64 anchors, of 65 ... 128, those the
 * wavefront kernel took instead, tile items, fragments in them, fragments handed back, deferred segments, those of them chained sixteen lanes
 * each, fragments compacted, fragments through the segment-wise kernels, segments to the wavefront kernel, fragments to the chain-order kernels,
 * fragments chained whole after them, size of the second round, fragments under AL_TEST_SEG_BIG, fragments of the fallback's virtual batches,
 * n_chain_fallback, lds_ok, tiles_ok, tile_from, the list positions of 1, 65 and 129 anchors, lmin.  Returns 0; -2: offsets out of order. */
int  al_dbg_chain(al_ctx_t *ctx, const uint64_t *anchors_xy, const uint64_t *a_off, const uint32_t *tie_flag, uint32_t *nu_out, uint64_t *u_out, uint32_t *uo_out, uint64_t *chained_xy, uint64_t *counts);
/* Tap (parity tests): the stage between chaining and extension -- a fragment's chains to its per-mate hits (mm_gen_regs, mm_set_parent,
 * mm_select_sub(_multi), mm_seg_gen, the per-mate mm_set_parent and the squeeze) -- on caller-supplied chains, through the host code the stage runs
 * for a batch: the chain-count classes and their k_regs_select launches, k_regs_heavy_classify and the k_regs_heavy tiles, k_regs_cap2 and the parts
 * of k_regs, on their streams, up to the stage's ST_REGS event; in a map-only context (AL_F_OUT_PAF without AL_F_CIGAR) on through k_map_only and
 * k_map_only_wave.  Needs a batch uploaded with al_batch_upload and NOT run (dummy reads of the wanted lengths and names will do).  In: what
 * al_dbg_chain puts out (nu, u, uo, chained_xy over a_off) and frag_rep[n_frag], the fragments' rep_len.  Out: reg_cnt / seg_na[n_reads]; regs_n0 and
 * frag_hash[n_frag] (regs_n0: kept hits, 0xfffffffe = finished by k_regs_heavy, 0xffffffff = left to k_regs, 0xfffffff1 ... 3 = the selection gave
 * up; all 0xffffffff when the selection kernels did not run); counts[17]: the list positions of 5, 65, 1025, 8193, 2049, 4097 and 257 chains, the
 * fragments per k_regs_heavy tile (12, 24, 48, 72, 200 hits), log-table misses, sort ties seen, whether the selection kernels ran, mates given to
 * k_map_only_wave, entries of the log table; sizes[2]: hits of all reads, records of the dense map-only output.  Returns 0; -2: a chain outside its
 * fragment's anchors or an anchor outside its read (nothing ran).
 * al_dbg_regs_fetch, after it: regs_out[n_regs] = the per-mate hits as 112-byte device records (id cnt rid score | qs qe rs re | parent subsc as mlen |
 * blen n_sub score0 hash | mapq flags ...; flags = split | rev << 2 | inv << 3 | sam_pri << 4 | proper << 5 | pe_thru << 6 | seg_split << 7 |
 * seg_id << 8 | split_inv << 16 | has_p << 17), read after read; seg_a_xy: the per-mate anchors, a_off[n_frag] of them (mate 0's of fragment f from
 * a_off[f], mate 1's seg_na[mate 0] further on; a hit's are [as, as + cnt) of its mate's); dense_out[n_dense]: the map-only output, same order. */
int  al_dbg_regs(al_ctx_t *ctx, const uint32_t *nu, const uint64_t *u, const uint32_t *uo, const uint64_t *chained_xy, const uint64_t *a_off, const int32_t *frag_rep,
                 uint32_t *reg_cnt, uint32_t *seg_na, uint32_t *regs_n0, uint32_t *frag_hash, uint64_t *counts, uint64_t *sizes);
int  al_dbg_regs_fetch(al_ctx_t *ctx, void *regs_out, uint64_t n_regs, uint64_t *seg_a_xy, void *dense_out, uint64_t n_dense);
/* Tap (parity tests): the extension stage -- a mate's hits and anchors to its final records: k_ext_prep(_wave), the DP job classes, k_ext_finish(_wave), the
 * monolithic k_align / k_align_long with their early, late and solo launches, k_compact -- on caller-supplied chains, through al_run_align_stage itself, run
 * to its end inside the loop that runs it again with twice the CIGAR arena while the arena overflows (the loop al_batch_run has).  Needs a batch uploaded
 * with al_batch_upload and NOT run, of the real reads, on an index of the contigs the anchors point into, and a context that is not map-only.  In: as
 * al_dbg_regs.  Afterwards the context is as al_batch_run leaves it: al_batch_fetch returns the records.  counts[29]: fragments left to the monolithic
 * kernel after prep and after the DP, whether those two launches were solo, whether the whole batch went through the monolithic kernel (AL_DBG bit 26, long
 * mode), long mode, the k_align instance's target tile (336, 512, 1024; 0: k_align_long), the job-slot thresholds of the wavefront forms of prep and finish
 * in effect (0: none), the fragments at or above each, the flanks done in closed form, the job slots, counters[7] (oversize and window bail-outs), log-table
 * misses, counters[9] of the last run (arena overflow), how often the stage ran again, the records, the arena words used, the DP jobs per class [10].  All of
 * it is what the host already holds or, read back here only, the job table the last run left: a batch run launches what it launched before.
 * Returns 0; -2: as al_dbg_regs, or an anchor whose k-mer leaves its contig, or a chain that changes contig or strand or does not ascend (nothing ran). */
int  al_dbg_align(al_ctx_t *ctx, const uint32_t *nu, const uint64_t *u, const uint32_t *uo, const uint64_t *chained_xy, const uint64_t *a_off, const int32_t *frag_rep, uint64_t *counts);
/* Tap (parity tests): the seed stage of a pass as a batch run launches it -- sketch, seed lookup, anchor collection, the sorts and the merges of the
 * flagged fragments, on their streams and in their order -- without the chaining.  Needs a batch uploaded with al_batch_upload.  list == NULL: the
 * first pass (mid_occ) on every fragment.  list[n_list], ascending fragment ids: the re-chain pass of those fragments with max_occ, in the place of
 * the list the first pass's chains would have selected; once, after a first pass of this tap on the same batch; needs max_occ > mid_occ; the merges
 * the first pass made ahead are taken as a run takes them.  The pass's results stay in the context for al_dbg_copy: "frag_na", "frag_nm",
 * "frag_rep", "a_off", "anchors", "tie_list" (per fragment: 0 sorted, 1 merged by a heap kernel, 2 taken from a merge made ahead), "mini" ...
 * counts[40] (may be NULL), fragments of this pass per sort kernel: k_anchor_sort_small; k_anchor_sort_reg <2,1,128> <4,1,256> <8,1,512> <16,1,512>
 * <8,4,1024> <16,4,1024> <16,8,1024>; k_anchor_sort<1024>; the run merge's fragments, tiles and passes; the device radix sort's fragments and
 * chunks; fragments flagged wholesale (rank_bits < 0); whether the keys are compact, rid_bits, pos_bits, rank_bits + 64; the pass's list length and
 * the list positions of 65, 129, 257, 513 anchors, of the block sorts' bound and of 2049, 4097 anchors and the device-wide sort's bound; then
 * from the device: this pass's heap merges, merges made ahead, how many of them this pass took, fragments on the merge kernels' list (flag word 1); the
 * heap merges by launch (each gets a counter word of its own in this tap): k_anchor_heap_lanes<2>, <1>, k_anchor_heap<0>, k_anchor_heap_wave,
 * k_anchor_heap<48>, <96>; the sketch form the first pass's arguments select (1 d_sketch<11>, 2 d_sketch<0>, 3 d_sketch_wide) and its position bits + 64.
 * Returns 0; -2: no first pass before the second, or a list out of order. */
int  al_dbg_seed(al_ctx_t *ctx, const uint32_t *list, int n_list, uint64_t *counts);

/* Self-test of the multi-lane output path (offset exchange + pwrite, or ordered turns) with synthetic blocks; needs no GPU. */
int  al_dbg_ordered_out_selftest(const char *path, int n_lanes, int n_batches, int use_offsets);
/* The radix-sort restatement (klib ksort.h radix_sort, unstable above 64 elements) in its serial and its wavefront form on the same
 * keys: both permutations of 0..n-1 come back; n <= 65535.  Test hook. */
int  al_dbg_rs_sort(int device, const uint64_t *keys, int n, uint16_t *order_serial, uint16_t *order_wave);
/* Self-test of the whole-file parallel FASTA loader of the index builders against the block reader: 0 = same names, lengths and
 * bytes, 1 = the loader declined the file (not a plain uncompressed FASTA), -1 = they differ; needs no GPU. */
int  al_dbg_fasta_selftest(const char *fn, int n_threads);
/* Self-test of the block-parallel FASTQ parser of the host driver against its serial kseq-grammar reader on one file: 0 = the same
 * records, -1 = they differ, -2 = the file cannot be opened; needs no GPU. */
int  al_dbg_fastq_selftest(const char *fn, int n_threads);
/* Self-test of the SAM record formatter the GPU runs (k_sam_len / k_sam_write; mm_write_sam3, format.c:387-544), compiled for the CPU:
 * n_frag random fragments formatted by it and by al_write_sam, `de:f:%.4f` checked against printf; returns the number of
 * differences (0 = identical); needs no GPU. */
int  al_dbg_sam_selftest(uint64_t seed, int n_frag);
/* The same for the PAF formatter (k_paf_len / k_paf_write; mm_write_paf3, format.c:304-330) against al_write_paf. */
int  al_dbg_paf_selftest(uint64_t seed, int n_frag);
/* The same for the BAM record formatter (k_bam_len / k_bam_write; al_dev_bam.h) against al_write_bam_rec: every record's bytes, the counted
 * length and, for the coordinate-sorted output, the records kept and their sort keys. */
int  al_dbg_bam_selftest(uint64_t seed, int n_frag);
/* The bits of the float that formatter stores as de:f for the "%.4f" digits q (the value q / 10000). */
uint32_t al_dbg_bam_de_bits(uint64_t q);

/* ---- device-resident batch API (bench / multi-GPU harness; inputs already in HBM when timing starts) ---- */
/* Pack + upload a batch; returns 0.  The batch stays resident until the next upload. */
int  al_batch_upload(al_ctx_t *ctx, int n_frag, const int *n_segs, const int *qlens, const char *const *seqs,
                     const char *const *qnames);
/* Same, for flat buffers: sequences concatenated in read order (not NUL-terminated), every read of fragment f
 * named "<name_prefix><first_index+f>" (BBMap rename.sh naming, extract_sequence.sh:18). */
int  al_batch_upload_flat(al_ctx_t *ctx, int n_frag, const int *n_segs, const int *qlens, const char *seq_concat,
                          const char *name_prefix, int64_t first_index);
/* Run the whole hot path (sketch .. alignment records) on the resident batch; results stay on device.
 * Returns 0, or AL_ERR_NOMEM when a device workspace for this batch could not be allocated (workspaces grow with the
 * number of seed hits: a batch of reads from high-copy repeats can need hundreds of bytes per hit).  The context gives its
 * batch workspaces back and stays usable: upload fewer fragments and run again -- the file drivers below halve the batch and retry on their own, the
 * way the reference's per-read loop (map.c:229-400) is unaffected by how many reads share a mini-batch.  Any other
 * non-zero value is a device error. */
#define AL_ERR_NOMEM (-12)
int  al_batch_run(al_ctx_t *ctx);
/* Fetch results of the last al_batch_run into host reg arrays (same contract as al_map_batch). */
int  al_batch_fetch(al_ctx_t *ctx, int *n_regs, al_reg1_t **regs, int *rep_len);

/* Device -> host copy of the flat result block of the last al_batch_run into page-locked buffers kept by the library (what the file
 * drivers do per batch); reports the records and bytes moved.  For timing the PCIe-inclusive rate. */
int  al_batch_fetch_flat(al_ctx_t *ctx, uint64_t *n_records, uint64_t *n_bytes);

/* ---- token batches: reads that are fixed-length windows of longer sequences, cut on the device ---- */
typedef struct al_winsrc_s al_winsrc_t;     /* source sequences, concatenated, packed 4 bit/base in the context's GPU memory */
al_winsrc_t *al_winsrc_create(al_ctx_t *ctx, const char *ascii, uint64_t n_bases);
void         al_winsrc_destroy(al_winsrc_t *src);
/* n_tok single-segment reads of read_len bases; read i = source bases [start[i], start[i] + read_len); qnames as in
 * al_batch_upload.  Then al_batch_run / al_batch_fetch as usual. */
int  al_batch_upload_windows(al_ctx_t *ctx, const al_winsrc_t *src, int n_tok, const uint64_t *start, int read_len, const char *const *qnames);
/* Whole stage: what AirLift does with gaps_to_fasta.py (tile every sequence of `gaps_fn` into read_size-base tokens every `skip`
 * bases, named <sequence>_<start>) followed by the single-end alignment of the tokens (align_gaps.sh:14-15); SAM on `out`. */
int  al_map_tokens_file(const al_idx_t *mi, const char *gaps_fn, int read_size, int skip, const al_mapopt_t *opt, int n_threads,
                        FILE *out, const char *rg, int device);
/* The same stage with the only thing AirLift reads from that SAM as its output (extract_regions.sh, run_pipeline.sh:62): the intervals
 * [POS - 1, POS - 1 + reference span) of every mapped record the SAM run would print, sorted as sort-bed sorts (contig name in byte order,
 * start, end) and merged as mergeBed merges (distance 0) -- on `regions` within each gap sequence of `gaps_fn`, the gaps one after the
 * other in file order; on `merged` across all of them.  BED lines "contig\tstart\tend\n".  Either FILE may be NULL, not both.  The
 * records stay on the device: the intervals are collected, sorted and merged there, no SAM text is made.  The tag and =/X options in
 * `opt` have no effect.  Return codes as al_map_tokens_file. */
int  al_map_tokens_regions(const al_idx_t *mi, const char *gaps_fn, int read_size, int skip, const al_mapopt_t *opt, int n_threads,
                           FILE *regions, FILE *merged, int device);
/* Test taps of the region merge: n caller-given intervals {group, rank (of the contig's name), start, end} through the device list and
 * its folds (al_dbg_regions_merge, on the current device) or through their host twin (al_dbg_regions_merge_host).  chunk > 0: the
 * intervals are appended `chunk` at a time with a fold after each append (the fold between batches); 0: all at once.  per_gap != 0: the
 * regions of every (group, rank); 0: merged across the groups (every group 0).  The o_* arrays have room for n; *n_out regions. */
int  al_dbg_regions_merge(uint64_t n, const uint32_t *group, const uint32_t *rank, const uint32_t *start, const uint32_t *end, uint64_t chunk, int per_gap,
                          uint32_t *o_group, uint32_t *o_rank, uint32_t *o_start, uint32_t *o_end, uint64_t *n_out);
int  al_dbg_regions_merge_host(uint64_t n, const uint32_t *group, const uint32_t *rank, const uint32_t *start, const uint32_t *end, uint64_t chunk, int per_gap,
                               uint32_t *o_group, uint32_t *o_rank, uint32_t *o_start, uint32_t *o_end, uint64_t *n_out);
/* The two stages above with the gaps BED in place of the gap FASTA: a row "name \t a \t b" of `bed_fn` (further columns ignored, empty lines skipped)
 * stands for what `samtools faidx REF name:a-b` prints for the indexed reference -- the header "name:a-b" from the literal text of the fields, the bases
 * [max(a, 1) - 1, min(b, contig length)) of contig `name` -- and is tiled as a sequence of GAPS.fa is.  The tokens are set up and cut on the device from
 * the index's own 4-bit reference, so SEQ of the SAM is upper-case ACGTN; every other column, and both BED outputs (group = BED row), are those of the
 * FASTA run over the equivalent GAPS.fa.  A row with fewer than three fields, a non-numeric a or b, b < a or a contig the index does not have is refused
 * with its file and line number (-1), before any device is opened.  Return codes otherwise as al_map_tokens_file / al_map_tokens_regions. */
int  al_map_tokens_bed_file(const al_idx_t *mi, const char *bed_fn, int read_size, int skip, const al_mapopt_t *opt, int n_threads,
                            FILE *out, const char *rg, int device);
int  al_map_tokens_bed_regions(const al_idx_t *mi, const char *bed_fn, int read_size, int skip, const al_mapopt_t *opt, int n_threads,
                               FILE *regions, FILE *merged, int device);
/* Test taps of the token set-up: n_rows regions given by their names ("name:a-b", NUL-terminated, one after the other in names[0, names_len)), first
 * bases src[] and lengths len[]; tokens [t0, t0 + n) of their table through k_tok_setup on the current device (al_dbg_tokens_table) or through its host
 * twin (al_dbg_tokens_table_host): o_start[i] the first base of token t0 + i's window, o_hash[i] its fragment hash.  o_first_tok (n_rows + 1) and
 * o_h_prefix (n_rows) receive the table when they are not NULL.  No index, no mapping.  -1: arguments, or tokens beyond the table. */
int  al_dbg_tokens_table(uint32_t n_rows, const char *names, size_t names_len, const uint64_t *src, const uint32_t *len, int read_size, int skip, int seed,
                         uint64_t t0, uint64_t n, uint64_t *o_start, uint32_t *o_hash, uint64_t *o_first_tok, uint32_t *o_h_prefix);
int  al_dbg_tokens_table_host(uint32_t n_rows, const char *names, size_t names_len, const uint64_t *src, const uint32_t *len, int read_size, int skip, int seed,
                              uint64_t t0, uint64_t n, uint64_t *o_start, uint32_t *o_hash, uint64_t *o_first_tok, uint32_t *o_h_prefix);

/* ---- the chain file's region logic (chain-beds, tokens --chain): 2_get_updated_regions_bed.py, get_constant_regions.py and get_retired_regions.py ----
 * Comments ('#' first), blank lines, headers "chain score tName tSize tStrand tStart tEnd qName qSize qStrand qStart qEnd id" and alignment lines
 * "size dt dq" / "size" of `chain_fn` are read on the host; the pad / clamp / sort / merge / invert of the three scripts runs on `device` (-1: the
 * default device), or with AL_CHAIN_HOST in `flags` through the kernels' host twin, which opens no device.  Inclusive rows "name\tstart\tend\n":
 *   gaps      the gaps between the blocks, padded by read_size + max_errors, clamped to the contig and merged where they overlap (2_get_updated_regions_bed.py)
 *   constant  the blocks as they are, contig by contig in order of first header (get_constant_regions.py)
 *   retired   what neither a block nor a row of `merged_fn` ("contig start end", the numbers as written), each padded by read_size, covers -- with the
 *             script's tail rule: the stretch behind a contig's last region is a row only when the contig already has one (get_retired_regions.py)
 * Any FILE may be NULL, not all; gaps needs max_errors >= 0, retired needs merged_fn.  Malformed input (a data line before the first header, a field
 * count other than 1 or 3, a non-numeric field, size 0, a line after a chain's 1-field line, tSize >= 2^31, a tStrand other than '+', a block or gap
 * that ends beyond tSize; a merged row with fewer than 3 fields, end < start, start beyond the contig, or a contig no header names) is refused as
 * FILE:LINE: reason with -1, before any device is opened.  The scripts' chatter on stdout is not printed. */
#define AL_CHAIN_HOST 1u
int  al_chain_beds(const char *chain_fn, int read_size, int max_errors, const char *merged_fn, FILE *gaps, FILE *constant, FILE *retired, unsigned flags, int device);
/* tokens with the chain file in place of the gaps BED: the gaps rows above are computed on the device and tiled exactly as al_map_tokens_bed_file /
 * al_map_tokens_bed_regions tile the rows of the file the script writes (a row "name a b" is the sequence name:a-b).  `gaps` (may be NULL) receives those
 * rows.  A tName the index lacks is refused (-1); a tSize that differs from the contig's length gets one notice, and rules the arithmetic.  _regions:
 * `retired` takes the run's merged regions from the device list where they lie; a merged contig no header names takes its length from the index.
 * `regions`, `merged`, `retired`, `constant` may each be NULL, not all four. */
int  al_map_tokens_chain_file(const al_idx_t *mi, const char *chain_fn, int max_errors, int read_size, int skip, const al_mapopt_t *opt, int n_threads,
                              FILE *out, const char *rg, int device, FILE *gaps);
int  al_map_tokens_chain_regions(const al_idx_t *mi, const char *chain_fn, int max_errors, int read_size, int skip, const al_mapopt_t *opt, int n_threads,
                                 FILE *regions, FILE *merged, int device, FILE *retired, FILE *constant, FILE *gaps);
/* Test taps of the region logic on a parsed line table: lines {chain, size, dt, three} in file order, chains {c_slot, c_tstart}, slots L[]; for the
 * retired step (n_retired != NULL) merged rows {m_slot, m_start, m_end} in the slots of that step, rslot_of[n_slot] the step's slot of every chain
 * slot and RL[n_rslot] the lengths.  Through the kernels on the current device (al_dbg_chainreg) or their host twin (al_dbg_chainreg_host).  Rows come
 * back as triples slot, start, end: o_gaps and o_constant have room for 3 * n numbers, o_retired for 6 * (n + n_m); an output whose count pointer is NULL
 * is not computed.  -1: arguments, or a table that breaks what the parser guarantees. */
int  al_dbg_chainreg(uint64_t n, const uint32_t *chain, const uint32_t *size, const uint32_t *dt, const uint32_t *three, uint32_t n_chain, const uint32_t *c_slot, const uint32_t *c_tstart,
                     uint32_t n_slot, const uint32_t *L, uint64_t n_m, const uint32_t *m_slot, const uint32_t *m_start, const uint32_t *m_end, uint32_t n_rslot, const uint32_t *rslot_of, const uint32_t *RL,
                     int R, int E, uint32_t *o_gaps, uint64_t *n_gaps, uint32_t *o_constant, uint64_t *n_constant, uint32_t *o_retired, uint64_t *n_retired);
int  al_dbg_chainreg_host(uint64_t n, const uint32_t *chain, const uint32_t *size, const uint32_t *dt, const uint32_t *three, uint32_t n_chain, const uint32_t *c_slot, const uint32_t *c_tstart,
                          uint32_t n_slot, const uint32_t *L, uint64_t n_m, const uint32_t *m_slot, const uint32_t *m_start, const uint32_t *m_end, uint32_t n_rslot, const uint32_t *rslot_of, const uint32_t *RL,
                          int R, int E, uint32_t *o_gaps, uint64_t *n_gaps, uint32_t *o_constant, uint64_t *n_constant, uint32_t *o_retired, uint64_t *n_retired);

/* ---- the exact chain file (chain-exact verify|build): run/1_build_exact_chain_file.py ----
 * The old reference (the headers' tName .. tEnd) and the new one (qName .. qEnd) are compared base by base over every block of `chain_fn` on `device` (-1:
 * the default device), or with AL_CHAIN_HOST in `flags` by the kernels' host twin, which opens no device.  `out` receives the bytes the script prints:
 *   AL_CEX_VERIFY  a line "mismatch: E errors in SIZE blocktarget: QNAME header: ..." per block with mismatches, or "PASS VERIFICATION"
 *   AL_CEX_BUILD   the chain file rebuilt: every block cut at its mismatches, stretches shorter than `min_region` (the script: 100) folded into the gaps,
 *                  heads and tails moved into the headers; chains in the script's order (first appearance of tName, of qName, of tStart)
 * Refused as FILE:LINE: reason with -1: what al_chain_beds refuses of a chain file (qStrand may be '-'), a header number that is none, a chain whose last
 * line is not 1-field, two headers with the same (tName, qName, tStart), a contig name twice in a FASTA, a 'U' or 'u' among the bases, on a '-' chain a
 * block that leaves the new contig or a new-side byte other than acgtnACGTN, and in build a name the FASTA lacks or a block that ends beyond its contig
 * (there the script prints a one-line message and no chain). */
#define AL_CEX_VERIFY 0
#define AL_CEX_BUILD 1
int  al_chain_exact(const char *old_fa, const char *new_fa, const char *chain_fn, int mode, int min_region, FILE *out, unsigned flags, int device);
/* Test taps of the comparison on two texts and a block table: blocks {chain, size, dt, dq, three} in output order, chains {c_old0, c_new0: the text
 * offsets of the first block's first base (c_new0: its last on the new side where c_dir is 1), c_dir}.  Through the kernels on the current device
 * (al_dbg_chainexact) or their host twin (al_dbg_chainexact_host).  o_cnt[n]: mismatches per block; *o_flag: 1 when a '-' block meets a new-side byte
 * other than acgtn -- then nothing else is said.  With `build`: the positions as pairs block, idx (room for cap_pos pairs), the lines after pass 1 and
 * after pass 2 as chain, size, dt, dq, three (room for cap_l1 / cap_l2 lines).  -1: arguments, or a table that breaks what the table builder
 * guarantees; -4: an output has too little room.  al_dbg_chainexact_tile: the bases of a block that one wavefront compares. */
int  al_dbg_chainexact(const uint8_t *old_text, uint64_t n_old, const uint8_t *new_text, uint64_t n_new, uint64_t n, const uint32_t *chain, const uint32_t *size, const uint32_t *dt, const uint32_t *dq,
                       const uint32_t *three, uint32_t n_chain, const uint64_t *c_old0, const uint64_t *c_new0, const uint32_t *c_dir, int build, int min_region, uint32_t *o_cnt, uint32_t *o_pos,
                       uint64_t cap_pos, uint64_t *n_pos, uint32_t *o_l1, uint64_t cap_l1, uint64_t *n_l1, uint32_t *o_l2, uint64_t cap_l2, uint64_t *n_l2, uint32_t *o_flag);
int  al_dbg_chainexact_host(const uint8_t *old_text, uint64_t n_old, const uint8_t *new_text, uint64_t n_new, uint64_t n, const uint32_t *chain, const uint32_t *size, const uint32_t *dt, const uint32_t *dq,
                            const uint32_t *three, uint32_t n_chain, const uint64_t *c_old0, const uint64_t *c_new0, const uint32_t *c_dir, int build, int min_region, uint32_t *o_cnt, uint32_t *o_pos,
                            uint64_t cap_pos, uint64_t *n_pos, uint32_t *o_l1, uint64_t cap_l1, uint64_t *n_l1, uint32_t *o_l2, uint64_t cap_l2, uint64_t *n_l2, uint32_t *o_flag);
uint32_t al_dbg_chainexact_tile(void);

/* ---- lift: the constant-region reads of a BAM moved across the chain file (run_pipeline.sh:92-95, FastRemap) ----
 * Every record of `bam_in` (a BGZF file) goes through the block table of `chain_fn` on `device` (-1: the default device): a mapped record that lies wholly
 * and uniquely inside one block of a '+' chain gets the new refID, pos and bin, its mate fields are lifted as a point, and it is written to `bam_out` in
 * input order; a mapped record that does not lift leaves the BAM and becomes a row "chrom s e name[.1|.2] MAPQ CIGAR" of `bed_out` (the six columns
 * extract-reads writes); an unmapped record is always kept.  The header's @SQ lines and reference list become the chain's qNames, an SO: value becomes
 * unsorted.  The function is stated in full in airlift_amd/csrc/al_dev_lift.h.  flags: AL_LIFT_HOST -- the kernels' host twin, no device is opened (it also
 * takes over, with a notice, where the device or its memory is refused); AL_LIFT_GPU_DEFLATE -- the packed records are deflated where they lie;
 * AL_LIFT_SORTED -- `bam_out` holds the same records, byte for byte, in coordinate order: by refID << 32 | pos after the lift, records without a refID last
 * (unmapped records stay: a placed one sorts at its lifted position), equal keys in input order; the header says SO:coordinate (a text without @HD gets the
 * line "@HD VN:1.6 SO:coordinate" first); `bed_out` is the same.  Each piece is put in order on the device -- sorted only when it is not in order already --
 * and the pieces are merged on the host, spilling merged runs to unlinked files in TMPDIR beyond AL_SORT_MEM bytes (0: never), as --sorted-bam does; the
 * merged bytes go through the compressor from host memory, with AL_LIFT_GPU_DEFLATE too.  The figures of the sort are on the AL_TIMING line only.
 * level: the BGZF level; n_threads: host threads of the compressor and of the twin's inflater; piece_bytes: inflated bytes per piece (0: the default).
 * 0; -1 with a message (a chain file refused as FILE:LINE: reason, a file that is no BGZF file, the wrong reference, I/O); -2 malformed BAM input, the
 * message names the record's offset in the inflated stream.  On an error the two output files are removed.  All device memory is released before the
 * return (stat->held == 0). */
#define AL_LIFT_HOST 1u
#define AL_LIFT_GPU_DEFLATE 2u
#define AL_LIFT_SORTED 4u
typedef struct {
	uint64_t kept, unlifted, unmapped_kept;   /* records: lifted and kept, gone to the BED, unmapped and kept */
	uint64_t pieces, bytes_in, held;          /* pieces walked, inflated bytes, device bytes of the call's account at return */
	double   read_s, up_s, inflate_s, walk_s, lift_s, down_s, deflate_s, wall_s;   /* file read, copy up, inflate, walk, lift + gather, copy down, deflate, wall */
	int      on_device;                       /* 1: the kernels ran; 0: the host twin */
} AlLiftStat;
int  al_lift_bam(const char *bam_in, const char *chain_fn, const char *bam_out, const char *bed_out, unsigned flags, int device, int n_threads, int level, size_t piece_bytes, AlLiftStat *stat);
/* Test taps: one uncompressed BAM stream (header and records) and a chain file through ONE pass of the kernels (al_dbg_lift) or of their host twin
 * (al_dbg_lift_host).  The text is the stream as given and the walk starts behind the header.  rec_off / verdict[0, out4[0]): offset and verdict (0 kept,
 * 1 unlifted, 2 unmapped and kept, 3.. refused) of every complete record; out4: records, offset of the first incomplete record, first refused record
 * (~0: none) and its code; packed: the kept records one behind the other; arena: per unlifted record a descriptor {name_len, n_cigar, MAPQ | flag << 8,
 * refID, s, 0, e (64 bits)}, the name and the CIGAR words, padded to 8 bytes.  0; -1: the device failed; -3: an array is too small (the counts are set);
 * -4: the chain file or the header is refused.  al_dbg_lift_window: the bytes of text k_bam_walk stages at a time. */
int  al_dbg_lift_host(const void *bam, size_t n, const char *chain_fn, uint32_t *rec_off, uint32_t *verdict, size_t rec_cap, uint64_t *out4, void *packed, size_t packed_cap, size_t *packed_n,
                      void *arena, size_t arena_cap, size_t *arena_n);
int  al_dbg_lift(int device, const void *bam, size_t n, const char *chain_fn, uint32_t *rec_off, uint32_t *verdict, size_t rec_cap, uint64_t *out4, void *packed, size_t packed_cap, size_t *packed_n,
                 void *arena, size_t arena_cap, size_t *arena_n, size_t *held);
uint32_t al_dbg_lift_window(void);
/* The same pass as AL_LIFT_SORTED makes it: packed holds the kept records in key order; perm[0, sort3[0]) (room for rec_cap): the record index of every
 * packed record; sort3: packed records, descents (positions i of the kept records, in input order, whose key is below the key of the one before), 1 when a
 * sort was launched (the twin: when it sorted) -- 0 for a piece without a descent.  tap_flags & 1: the sort's temporaries count as refused, the order is
 * then made on the host and no sort is launched. */
int  al_dbg_lift_sorted_host(const void *bam, size_t n, const char *chain_fn, uint32_t *rec_off, uint32_t *verdict, size_t rec_cap, uint64_t *out4, void *packed, size_t packed_cap, size_t *packed_n,
                             void *arena, size_t arena_cap, size_t *arena_n, uint32_t *perm, uint64_t *sort3);
int  al_dbg_lift_sorted(int device, const void *bam, size_t n, const char *chain_fn, uint32_t *rec_off, uint32_t *verdict, size_t rec_cap, uint64_t *out4, void *packed, size_t packed_cap, size_t *packed_n,
                        void *arena, size_t arena_cap, size_t *arena_n, uint32_t *perm, uint64_t *sort3, unsigned tap_flags, size_t *held);

/* ---- merge: 2 to 8 coordinate-sorted BAMs merged into one (run_pipeline.sh:116 and :119, samtools merge) ----
 * Every record of the BGZF files `bam_in[0 .. n_in)`, each in coordinate order, written to `bam_out` in non-decreasing order of the key refID << 32 | pos
 * (records without a refID last); among equal keys the records of an earlier input come first, within one input the input's order holds.  The output's
 * reference list is input 1's with the contigs only later inputs name appended; refID and next_refID of a later input's records are translated, every other
 * byte of a record is as read.  The header text is input 1's with SO:coordinate, then the later inputs' lines that are not yet present (a colliding @PG ID gets
 * the suffix .K, K the input's number; a colliding @RG ID is refused).  An input that is not in coordinate order, a contig with two lengths, and a later input
 * whose contigs stand in another order than the merged list are refused.  The function is stated in full in airlift_amd/csrc/al_dev_merge.h.  flags:
 * AL_MERGE_HOST -- the kernels' host twin, no device is opened (it also takes over, with a notice, where the device or its memory is refused);
 * AL_MERGE_GPU_DEFLATE -- the packed records are deflated where they lie.  level: 0-9 of the host compressor; piece_bytes: inflated bytes per refill of an
 * input's window (0: 8 MB).  `bam_out` is unlinked on failure.  0; -1 with a message on stderr; -2 refused input (unsorted, malformed, headers that do not
 * merge), its message on stderr.  With AL_TIMING=1 one line on stderr ends in "device bytes held at return: N". */
#define AL_MERGE_HOST 1u
#define AL_MERGE_GPU_DEFLATE 2u
typedef struct {
	uint64_t n_in, records, rounds, refills, bytes_in, held;   /* inputs, records written, rounds of the merge, window refills, inflated bytes, device bytes of the call's account at return */
	uint64_t records_in[8];                   /* records per input */
	double   read_s, up_s, inflate_s, walk_s, key_s, merge_s, gather_s, down_s, deflate_s, wall_s;   /* file read, copy up, inflate, walk, keys, bounds + merge, gather, copy down, deflate, wall */
	int      on_device;                       /* 1: the kernels ran; 0: the host twin */
} AlMergeStat;
int  al_merge_bams(const char *const *bam_in, int n_in, const char *bam_out, unsigned flags, int device, int n_threads, int level, size_t piece_bytes, AlMergeStat *stat);
/* Test taps: k uncompressed BAM streams (header and records) through the round loop of the kernels (al_dbg_merge) or of their host twin (al_dbg_merge_host).
 * piece: bytes per refill of an input's window; 0: every stream whole, which makes ONE round with every input at eof.  tags / keys[0, *n_out) and
 * packed[0, *packed_n): tag (input << 28 | record index in the input's window of that round), key and bytes of every merged record, round behind round;
 * *rounds: the rounds.  0; -1 a device failure; -2 unsorted or malformed input (its message printed); -3 the arrays are too small (the counts are set);
 * -4 a header is refused.  *held: device bytes of the tap's account at return.  al_dbg_merge_tile: AL_MERGE_TILE, the outputs of one k_merge_tile block. */
int  al_dbg_merge_host(const void *const *bam, const size_t *n, int k, size_t piece, uint32_t *tags, uint64_t *keys, size_t rec_cap, size_t *n_out, void *packed, size_t packed_cap, size_t *packed_n, uint64_t *rounds);
int  al_dbg_merge(int device, const void *const *bam, const size_t *n, int k, size_t piece, uint32_t *tags, uint64_t *keys, size_t rec_cap, size_t *n_out, void *packed, size_t packed_cap, size_t *packed_n, uint64_t *rounds,
                  size_t *held);
uint32_t al_dbg_merge_tile(void);

/* ---- bam-index: the BAI of a coordinate-sorted BAM (run_pipeline.sh:9, :95 and :119, samtools index) ----
 * The BGZF file `bam`, in coordinate order as `merge` requires it, is inflated and walked in pieces on `device` (-1: the default device) and its index is
 * written to `bai` (NULL: `bam` + ".bai") through a temporary name beside it.  The index is defined by the rules of airlift_amd/csrc/al_dev_bai.h -- bins by
 * reg2bin of [max(pos, 0), + reflen), one chunk per run of records of one bin, bins not folded into their parents, the linear index, pseudo-bin 37450 and
 * n_no_coor -- and answers the query procedure of the SAM specification; byte parity with samtools index is not claimed.  flags: AL_BAI_HOST -- the kernels'
 * host twin, no device is opened (it also takes over, with a notice, where the device or its memory is refused).  n_threads: host threads of the twin's
 * inflater; piece_bytes: inflated bytes per piece (0: 8 MB).  0; -1 with a message on stderr; -2 refused input (not in coordinate order, malformed, a record
 * that ends beyond 2^29 or beyond its contig), its message on stderr.  No output file is left behind on failure.  With AL_TIMING=1 one line on stderr ends in
 * "device bytes held at return: N".  AL_MERGE_WRITE_INDEX / AL_LIFT_WRITE_INDEX (the latter with AL_LIFT_SORTED only): the same function over `bam_out` once
 * it is closed, with the call's backend, written to `bam_out` + ".bai". */
#define AL_BAI_HOST 1u
#define AL_MERGE_WRITE_INDEX 4u
#define AL_LIFT_WRITE_INDEX 8u
typedef struct {
	uint64_t records, unplaced, pieces, bytes_in, chunks, bai_bytes, held;   /* records, those without a refID, pieces walked, inflated bytes, chunks written (pseudo-bins apart), bytes of the index, device bytes of the call's account at return */
	double   read_s, up_s, inflate_s, walk_s, key_s, assemble_s, wall_s;    /* file read, copy up, inflate, walk, keys + runs + linear index, host assembly and write, wall */
	int      on_device;                       /* 1: the kernels ran; 0: the host twin */
} AlBaiStat;
int  al_index_bam(const char *bam, const char *bai, unsigned flags, int device, int n_threads, size_t piece_bytes, AlBaiStat *stat);
/* Test taps: one uncompressed BAM stream (header and records) with the table of the BGZF members it would lie in -- file offset, stream offset and isize of
 * each, file_end: the file offset behind the last of them -- through the piece loop of the kernels (al_dbg_bai) or of their host twin (al_dbg_bai_host) with
 * pieces of `piece` bytes (0: the stream whole).  bai[0, *bai_n): the index (room for bai_cap bytes).  0; -1 a device failure; -2 refused input (its message
 * printed); -3 bai_cap is too small (*bai_n is set); -4 the header is refused.  *held: device bytes of the tap's account at return. */
int  al_dbg_bai_host(const void *bam, size_t n, const uint64_t *m_file, const uint64_t *m_stream, const uint32_t *m_isize, size_t n_mem, uint64_t file_end, size_t piece, void *bai, size_t bai_cap, size_t *bai_n);
int  al_dbg_bai(int device, const void *bam, size_t n, const uint64_t *m_file, const uint64_t *m_stream, const uint32_t *m_isize, size_t n_mem, uint64_t file_end, size_t piece, void *bai, size_t bai_cap, size_t *bai_n,
                size_t *held);

/* per-batch work counters + per-kernel HIP-event times of the last al_batch_run */
typedef struct {
	uint64_t n_frag, n_reads, n_bases;
	uint64_t n_mini, n_anchor, n_chain, n_regs_aln, n_refbases, n_cigar, n_rechain, n_heap_fallback, n_sort_tie_flag;
	uint64_t bytes_in, bytes_out;
	double   algorithmic_bytes;       /* SURVEY.md §8(d) formula evaluated with the counters above */
	float    ms_total;                /* HIP events around the whole device pipeline */
	float    ms_kernel[40];           /* HIP-event time per pipeline interval, see al_stage_name() / al_stage_kernel() */
	int      n_stage;
	float    ms_side_stream;          /* exact (serial) heap merge + whole-fragment chaining of the fragments with equal-x anchors: runs on a side stream, overlapped with the intervals above */
	uint64_t n_chain_fallback;        /* fragments re-chained whole because of equal-x chain starts among more than 64 chains */
	uint64_t dp_jobs[10];             /* extension DP jobs per class (lane 16/32/64 targets, group DP of 1/2/4/8/22/32 16-column blocks, LDS rows) ... */
	uint64_t dp_target_bases[10];     /* ... and the reference-window bases of those jobs: the W term of the algorithmic bytes, per DP kernel */
} al_batch_stat_t;
void al_batch_stat(const al_ctx_t *ctx, al_batch_stat_t *st);
const char *al_stage_name(int i);
/* the kernel that runs in interval i (as rocprofv3 --kernel-trace names it); "" where an interval is a few small launches */
const char *al_stage_kernel(int i);

/* ---- the fork's as-shipped observable: number of seed clusters that would go on to alignment ---- */
/* Seed stages only on the resident batch (upload it with one segment per fragment, as the fork's main loop maps read by read,
 * main.c:384-391); *total gets the batch's count (map.c:299-312). */
int  al_batch_count_candidates(al_ctx_t *ctx, int64_t *total);
/* Whole file: the value the unmodified fork prints as "Total No. of Mappings before alignment (verification)" (main.c:417).
 * Returns 0, negative on error. */
int  al_count_candidates_file(const al_idx_t *mi, const char *fn, const al_mapopt_t *opt, int n_threads, int device, int64_t *total);

/* the pre-alignment filters of the bundled mrFAST fork applied to those candidates, on the device (al_prefilter.hip): the
 * adjacency filter (MrFAST.c:1741-1764: every other seed of the read looked up at the position the candidate predicts; more than adj_e
 * absent seeds reject) and GreedySnake (GreedySnake.c:52-200 with EditThreshold snake_e, KmerSize snake_k, IterationNo snake_iter).
 * out4: candidates (= the count above), kept by adjacency, kept by GreedySnake, kept by both.  Resident batch of single-segment
 * fragments (first, mid_occ, seeding pass); the alignment path does not use it. */
int  al_batch_prefilter(al_ctx_t *ctx, int adj_e, int snake_e, int snake_k, int snake_iter, int64_t *out4);
/* ... and every candidate's two decisions: dec[0 .. min(out4[0], dec_cap)) = fragment << 32 | first anchor of the candidate's cluster << 2 |
 * kept by the adjacency filter << 1 | kept by GreedySnake (no particular order) */
int  al_batch_prefilter_decisions(al_ctx_t *ctx, int adj_e, int snake_e, int snake_k, int snake_iter, int64_t *out4, uint64_t *dec, int64_t dec_cap);
int  al_count_candidates_file_filtered(const al_idx_t *mi, const char *fn, const al_mapopt_t *opt, int n_threads, int device,
                                       int adj_e, int snake_e, int snake_k, int snake_iter, int64_t *out4);

/* ---- stage taps for parity tests (analogue of --print-seeds, map.c:333-338,381-385) ---- */
/* minimizers of read i of the resident batch: returns count, writes up to cap records (x = hash<<8|span, y = i<<32|pos<<1|strand) */
int  al_dbg_minimizers(al_ctx_t *ctx, int read_idx, uint64_t *xy, int cap);
/* sorted anchors ("SD") and chained anchors ("CN") of fragment f after al_batch_run; x,y interleaved */
int  al_dbg_anchors(al_ctx_t *ctx, int frag_idx, uint64_t *xy, int cap, int *rep_len);
int  al_dbg_chains(al_ctx_t *ctx, int frag_idx, uint64_t *u, int cap_u, uint64_t *xy, int cap_a);
/* a8 ALSER counter (map.c:299-312) for every read of the resident batch mapped as single segments */
int  al_dbg_alser_count(al_ctx_t *ctx, int64_t *total);
/* bulk copy of a named device array of the resident batch (tests); returns bytes copied or -1 */
int64_t al_dbg_copy(al_ctx_t *ctx, const char *name, void *dst, int64_t max_bytes);

/* SAM text (format.c:116-135, 387-544) */
#define AL_MM_VERSION "2.17-r954-dirty"   /* MM_VERSION of the fork (main.c:16): the version whose records this path reproduces */
/* the `ver` and `argc, argv` arguments of mm_write_sam_hdr (format.c:116-135; main.c:369 passes MM_VERSION and its own
 * argv): `\tVN:<ver>` and `\tCL:minimap2 <argv[1..]>` appended to the @PG line of every header written afterwards.
 * Process-wide; NULL / argc <= 1 leave the respective part out (the default). */
void al_set_program_line(const char *ver, int argc, char *const *argv);
int  al_write_sam_hdr(FILE *out, const al_idx_t *mi, const char *rg, char *rg_id_out /* >=256 bytes or NULL */);
int  al_write_sam(char *buf, size_t cap, const al_idx_t *mi, const char *qname, int l_seq, const char *seq, const char *qual,
                  int seg_idx, int reg_idx, int n_seg, const int *n_regss, const al_reg1_t *const *regss,
                  const char *rg_id, int rep_len);

/* mm_write_paf3 (format.c:304-330) for one hit r of the read `qname` (l_seq bases) as al_map_frag returned it; r == NULL: the line of a read
 * without hits (--paf-no-hit).  opt_flag: AL_F_OUT_CG prints cg:Z:, AL_F_OUT_MD / AL_F_OUT_CS name the tag `tag` holds (the value al_gen_MD /
 * al_gen_cs made, or NULL for none); both only on a record with a CIGAR.  rep_len < 0 leaves rl:i: out.  The line ends with '\n' (the fork's
 * mm_err_puts adds it).  Returns the length, -1 if cap is too small. */
int  al_write_paf(char *buf, size_t cap, const al_idx_t *mi, const char *qname, int l_seq, const al_reg1_t *r, int64_t opt_flag, int rep_len, const char *tag);

/* mm_gen_cs / mm_gen_MD (minimap.h:363-364, format.c:137-214): the cs:Z / MD:Z value (no tag prefix) of one record r as al_map_frag
 * returned it, for the read `seq` in sequencing orientation.  no_iden != 0: short cs (":len"), else long ("=BASES").  *buf is malloc()ed /
 * realloc()ed to fit (*max_len its size); returns the string length, -1 on error.  km is ignored.  The reference window comes from the
 * index's host copy when it has one (al_idx_build, al_idx_str, al_idx_load), otherwise [rs, re) is copied from the device index.
 * This is the slow path for API callers: the file drivers (--MD / --cs) compute the tags on the device for a whole batch. */
int  al_gen_cs(void *km, char **buf, int *max_len, const al_idx_t *mi, const al_reg1_t *r, const char *seq, int no_iden);
int  al_gen_MD(void *km, char **buf, int *max_len, const al_idx_t *mi, const al_reg1_t *r, const char *seq);

const char *al_version(void);

/* Device memory reserve (no reference analogue: kalloc's per-thread arenas, kalloc.c:38-205 / map.c:13-36, are the nearest thing).  Starts a
 * thread that obtains `bytes` of memory on `device` (< 0: LOCAL_RANK or 0) in a few large chunks and returns at once; every device range the
 * library uses afterwards -- index arrays, the index builder's temporaries, the mapping contexts' workspaces -- is served from those chunks
 * (requests that find no room fall back to the driver).  Meant to be called before al_idx_build_device so that obtaining the memory overlaps
 * the FASTA load and the index build.  One reserve per process; 0, or -1 if there is no usable device / a reserve on another device exists.
 * al_device_reserve_for_run sizes it from the reference and read files (bytes it asked for, 0 = run too small to be worth it, -1 = error). */
int al_device_reserve(int device, uint64_t bytes);
int64_t al_device_reserve_for_run(int device, const char *ref_fn, int n_fn, const char *const *fn);
uint64_t al_device_reserve_peak(void);        /* largest number of bytes in use at once so far (0 without a reserve) */
void al_device_reserve_reset_peak(void);
void al_device_reserve_report(FILE *fp);      /* one line: chunks, time, peak use */

#ifdef __cplusplus
}
#endif
#endif

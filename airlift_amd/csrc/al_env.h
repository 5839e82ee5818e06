// al_env.h -- every environment variable the library and the CLI read: name, type, default, parse rule and what it does, in one table (DESIGN.md 8 lists the
// names; the detail is here).  Host only: no HIP include, so that a plain C++ program can include it -- tests/csrc/env_main.cpp prints the table.
// Nothing under csrc/ calls getenv outside this header.  A variable is read at one of three times:
//   process   struct AlEnv, read once at the first call of al_env() and constant from then on: set these before the first call into the library
//   context   struct AlEnvCtx, read anew by every al_env_ctx() call: al_ctx_init copies it into the context's AlParams (tests set these between contexts)
//   call      the small functions at the end, read at every call: what the process launcher or the system sets (RANK, WORLD_SIZE, LOCAL_RANK, the run id,
//             TMPDIR), and the four variables the CLI and the library's self-tests set themselves while the process runs
// A row is one variable: field, parse rule with the default, and what the switch does.  The rule for "on" differs from switch to switch, and a row's comment
// names it: present (set to anything, the empty string included), non-zero, equals 1, or on unless 0 -- atoi() semantics throughout, so the empty string and
// a non-number count as 0.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <limits.h>
#include <algorithm>
#include <initializer_list>
#include <optional>

// ---- parse helpers ---------------------------------------------------------------------------------------------------------------------------------------
inline bool al_env_present(const char *k) { return getenv(k) != nullptr; }
inline int al_env_int(const char *k, int dflt) { const char *v = getenv(k); return v ? atoi(v) : dflt; }
inline int al_env_positive(const char *k, int dflt) { const int v = al_env_int(k, 0); return v > 0 ? v : dflt; }
inline long long al_env_ll(const char *k, long long dflt) { const char *v = getenv(k); return v ? atoll(v) : dflt; }
inline double al_env_double(const char *k, double dflt) { const char *v = getenv(k); return v ? atof(v) : dflt; }
inline uint64_t al_env_u64(const char *k, uint64_t dflt) { const char *v = getenv(k); return v ? (uint64_t)strtoull(v, nullptr, 10) : dflt; }
inline std::optional<int> al_env_opt_int(const char *k, int lo = INT_MIN, int hi = INT_MAX) { const char *v = getenv(k); return v ? std::optional<int>(std::max(lo, std::min(hi, atoi(v)))) : std::nullopt; }
inline std::optional<double> al_env_opt_double(const char *k) { const char *v = getenv(k); return v ? std::optional<double>(atof(v)) : std::nullopt; }

// ---- process ---------------------------------------------------------------------------------------------------------------------------------------------
// A std::optional field is a variable whose absence differs from every value (the default depends on the input, or absence takes another path); a
// const char * field is the variable's text (nullptr when unset) where the site parses it further.
struct AlEnv {
	// -- run time
	bool trace = al_env_present("AL_TRACE");                               // AL_TRACE (present): per-stage trace lines on stderr; some sites synchronise their stream to report a kernel's status
	bool timing = al_env_present("AL_TIMING");                             // AL_TIMING (present): timing and sizing reports on stderr
	bool timing_nonzero = al_env_int("AL_TIMING", 0) != 0;                 // AL_TIMING (non-zero): the second rule of the same variable -- only the first context's "streams: ..." line uses it
	bool trace_alloc = al_env_present("AL_TRACE_ALLOC");                   // AL_TRACE_ALLOC (present): device allocations of >= 32 MB listed with their call site
	bool serial_parse = al_env_present("AL_SERIAL_PARSE");                 // AL_SERIAL_PARSE (present): the serial FASTA / FASTQ readers instead of the block parsers
	std::optional<int> idx_threads = al_env_opt_int("AL_IDX_THREADS");     // AL_IDX_THREADS: host threads of the device index build (unset: the hardware's, at most 32)
	bool pg_plain = al_env_present("AL_PG_PLAIN");                         // AL_PG_PLAIN (present): bare @PG line, without version and command line
	bool no_rccl = al_env_present("AL_NO_RCCL");                           // AL_NO_RCCL (present): block offsets of a multi-GPU / multi-process run exchanged without RCCL
	bool host_io = al_env_present("AL_HOST_IO");                           // AL_HOST_IO (present): the host driver instead of the stream driver
	bool host_index = al_env_present("AL_HOST_INDEX");                     // AL_HOST_INDEX (present): the index built on the host
	bool no_reserve = al_env_present("AL_NO_RESERVE");                     // AL_NO_RESERVE (present): no device memory reserve for a file-to-file run
	std::optional<double> reserve_kb_per_read = al_env_opt_double("AL_RESERVE_KB_PER_READ"); // AL_RESERVE_KB_PER_READ: workspace per read the reserve is sized with (unset: 12 / 40 / 85 by the reference's size)
	double pool_chunk_gb = al_env_double("AL_POOL_CHUNK_GB", 0.0);         // AL_POOL_CHUNK_GB: chunk size of the reserve (<= 0: a sixth of the target, 2 ... 24 GB)
	int hbm_margin_mb = std::max(0, al_env_int("AL_HBM_MARGIN_MB", 2048)); // AL_HBM_MARGIN_MB (>= 0): what a device allocation must leave free for the runtime
	double rank_timeout = al_env_double("AL_RANK_TIMEOUT", 600.0);         // AL_RANK_TIMEOUT: seconds a rank waits for the others when the caller gives no timeout
	bool no_fast_exit = al_env_present("AL_NO_FAST_EXIT");                 // AL_NO_FAST_EXIT (present): the CLI returns from main instead of _exit (profilers flush from exit handlers)
	std::optional<int> dbg_frag = al_env_opt_int("AL_DBG_FRAG");           // AL_DBG_FRAG: debugging aid, the chain_post result of this fragment of every batch on stderr
	const char *gpu_max_hw_queues = getenv("GPU_MAX_HW_QUEUES");           // GPU_MAX_HW_QUEUES: only ever read, never set -- a context creates min(10, this) streams (al_stream_count)

	// -- stream driver
	std::optional<int> slots = al_env_opt_int("AL_SLOTS", 2, 8);           // AL_SLOTS (2 ... 8): text / SAM buffer sets per GPU (unset: 4 for a long input, else 5)
	std::optional<int> ctxs = al_env_opt_int("AL_CTXS");                   // AL_CTXS: mapping contexts per GPU (unset: 2 for a long input, else 3); the site clamps it to 1 ... slots
	int piece_mb = std::max(1, al_env_int("AL_PIECE_MB", 8));              // AL_PIECE_MB (>= 1): input piece
	int out_piece_mb = std::max(1, al_env_int("AL_OUT_PIECE_MB", 32));     // AL_OUT_PIECE_MB (>= 1): page-locked output piece
	int inflate_piece_kb = al_env_positive("AL_INFLATE_PIECE_KB", 16384);           // AL_INFLATE_PIECE_KB (> 0, else the default): file piece of --gpu-inflate
	std::optional<int> batch_reads = al_env_opt_int("AL_BATCH_READS", 2);  // AL_BATCH_READS (>= 2): fixed batches of this many reads, no probes
	double long_batch = al_env_double("AL_LONG_BATCH", 0.0);               // AL_LONG_BATCH: reads per batch of a long input (<= 0: 524 288, 2^20 from long_batch_big_from reads); also sizes the reserve
	double long_batch_big_from = al_env_double("AL_LONG_BATCH_BIG_FROM", 2.0e8); // AL_LONG_BATCH_BIG_FROM: reads from which a long input gets the 2^20-read batch
	std::optional<int> probe_reads = al_env_opt_int("AL_PROBE_READS", 2);  // AL_PROBE_READS (>= 2): reads of the first batch (unset: 32768); set, the run keeps its two probes
	std::optional<int> probe_mult = al_env_opt_int("AL_PROBE_MULT", 1);    // AL_PROBE_MULT (>= 1): the second batch as a multiple of the probe (unset: 4 or 8 by input and allocation rate)
	bool two_probes = al_env_present("AL_TWO_PROBES");                     // AL_TWO_PROBES (present): a long input keeps the small first batch
	double alloc_gbs = al_env_double("AL_ALLOC_GBS", 30.0);                // AL_ALLOC_GBS: GB/s at which the batch sizing assumes first-touch device memory
	double batch_ms = al_env_double("AL_BATCH_MS", 25.0);                  // AL_BATCH_MS: fixed cost of a batch the sizing assumes
	const char *streams = getenv("AL_STREAMS");                            // AL_STREAMS (text: al_stream_count): physical streams of a mapping context, 1 ... 10
	const char *stream_map = getenv("AL_STREAM_MAP");                      // AL_STREAM_MAP (text: al_stream_map_parse): experiments, an explicit role -> stream map

	// -- tests: paths forced on, thresholds lowered, fall-backs forced (results stay valid)
	const char *test_poison = getenv("AL_TEST_POISON");                    // AL_TEST_POISON (text: byte): every new device range filled with it
	const char *test_poison_only = getenv("AL_TEST_POISON_ONLY");          // AL_TEST_POISON_ONLY (text: n): only the n-th allocation of the process
	bool test_poison_log = al_env_present("AL_TEST_POISON_LOG");           // AL_TEST_POISON_LOG (present): sequence number and size of every allocation on stderr
	bool test_guard = al_env_present("AL_TEST_GUARD");                     // AL_TEST_GUARD (present): 4 KB guard zones around every device range, checked on free and after a batch
	const char *test_sort_blk = getenv("AL_TEST_SORT_BLK");                // AL_TEST_SORT_BLK (text): smallest anchor count that goes to the block sort
	const char *test_sort_big = getenv("AL_TEST_SORT_BIG");                // AL_TEST_SORT_BIG (text): smallest anchor count that goes to the device-wide sort
	const char *test_big_chunk = getenv("AL_TEST_BIG_CHUNK");              // AL_TEST_BIG_CHUNK (text): fragments per device-wide sort
	const char *test_run = getenv("AL_TEST_RUN");                          // AL_TEST_RUN (text: "<run>,<tile>"): shorter runs and merge tiles of the run merge
	const char *test_nomem_above = getenv("AL_TEST_NOMEM_ABOVE");          // AL_TEST_NOMEM_ABOVE (text: n): batches of more fragments are reported as out of memory
	const char *test_scrub = getenv("AL_TEST_SCRUB");                      // AL_TEST_SCRUB (text: byte): the hit arrays filled with it before the regs stage
	bool test_deflate_nomem = al_env_present("AL_TEST_DEFLATE_NOMEM");     // AL_TEST_DEFLATE_NOMEM (present): every device-buffer request of the BGZF compressor refused
	bool test_inflate_nomem = al_env_present("AL_TEST_INFLATE_NOMEM");     // AL_TEST_INFLATE_NOMEM (present): the device-buffer request of the BGZF reader refused
	bool test_inflate_host = al_env_int("AL_TEST_INFLATE_HOST", 0) != 0;   // AL_TEST_INFLATE_HOST (non-zero): the reader's host backend without asking the device, and without the notice
	bool test_tile_all = al_env_present("AL_TEST_TILE_ALL");               // AL_TEST_TILE_ALL (present): every fragment through the tile kernel
	bool test_tile_fb = al_env_present("AL_TEST_TILE_FB");                 // AL_TEST_TILE_FB (present): the tile kernel hands every fragment back
	std::optional<int> test_seg_big = al_env_opt_int("AL_TEST_SEG_BIG");   // AL_TEST_SEG_BIG: segment bound of the eight-wavefront forms (unset: 8192, by list position); set, every fragment takes them
	int test_heap_wave = al_env_int("AL_TEST_HEAP_WAVE", -1);              // AL_TEST_HEAP_WAVE: anchors from which a heap merge takes the wavefront form (negative: 8192 / 16384 by batch)
	int chain_coop = al_env_int("AL_CHAIN_COOP", -1);                      // AL_CHAIN_COOP: 0 never / 1 always the sixteen-lane chaining kernel (else: thin classes only)
	bool chain_ovl = al_env_int("AL_CHAIN_OVL", 1) != 0;                   // AL_CHAIN_OVL (on unless 0): lane chaining of the small fragments beside the sorts
	bool chain_ovl2 = al_env_int("AL_CHAIN_OVL2", 1) != 0;                 // AL_CHAIN_OVL2 (on unless 0): chaining classes on two streams in turn
	uint32_t chain_wave_max = (uint32_t)al_env_int("AL_CHAIN_WAVE_MAX", 8192); // AL_CHAIN_WAVE_MAX: classes thinner than this go to the wavefront kernel (0 = never, large = always)
	std::optional<int> prep_heavy = al_env_opt_int("AL_PREP_HEAVY");       // AL_PREP_HEAVY: jobs from which k_ext_prep takes the wavefront form (unset: the kernel file's constant; 0: never)
	int fin_heavy = al_env_int("AL_FIN_HEAVY", -1);                        // AL_FIN_HEAVY: the same for k_ext_finish (negative: by batch size; 0: never)
	int regs_split = al_env_int("AL_REGS_SPLIT", 1);                       // AL_REGS_SPLIT: bit 0, 257 ... 1024 chains sorted and passed over by two kernels
	bool heap_old = al_env_int("AL_HEAP_OLD", 0) == 1;                     // AL_HEAP_OLD (equals 1): the serial heap merges, and no merges ahead of the re-chain pass
	bool spec_merge = al_env_int("AL_SPEC_MERGE", 1) != 0;                 // AL_SPEC_MERGE (on unless 0): giant-fragment merges made ahead of the re-chain pass
	std::optional<int> spec_min = al_env_opt_int("AL_SPEC_MIN");           // AL_SPEC_MIN: smallest anchor count that gets such a merge (unset: 49152); set, they are made for every batch
	bool dp_pk = al_env_int("AL_DP_PK", 1) != 0;                           // AL_DP_PK (on unless 0): the two-cells-per-lane DP where its arithmetic holds
	bool dp_pk32 = al_env_int("AL_DP_PK32", 1) != 0;                       // AL_DP_PK32 (on unless 0): that form for the 32-block class too
	int big_merge = al_env_int("AL_BIG_MERGE", 1);                         // AL_BIG_MERGE: 0 radix everywhere, 1 run merge everywhere, 2 run merge in the re-chain pass only
	int order_block = al_env_int("AL_ORDER_BLOCK", 128);                   // AL_ORDER_BLOCK: chains from which a block of 16 wavefronts restates a fragment's chain order
	long long dp_conc = al_env_ll("AL_DP_CONC", 700000);                   // AL_DP_CONC: jobs below which the DP classes run side by side on four streams (0: never)

	// -- experiments
	bool side_prio = al_env_int("AL_SIDE_PRIO", 0) == 1;                   // AL_SIDE_PRIO (equals 1): the side streams at the highest stream priority
	bool dp_no_split = al_env_present("AL_DP_NO_SPLIT");                   // AL_DP_NO_SPLIT (present): the 9 ... 22-block DP class in one launch
	int cap4 = al_env_int("AL_CAP4", 4096), cap8 = al_env_int("AL_CAP8", 4096), cap22 = al_env_int("AL_CAP22", 3072);   // most blocks a DP class of up to 4 / 8 / 22-block jobs launches
	int grow_div = std::max(1, al_env_int("AL_GROW_DIV", 8));              // AL_GROW_DIV (>= 1): headroom of a large grow-only device array, 1 / this
};

inline const AlEnv &al_env() { static const AlEnv e; return e; }

// ---- context ---------------------------------------------------------------------------------------------------------------------------------------------
struct AlEnvCtx {
	int dbg = al_env_int("AL_DBG", 0);                                     // AL_DBG: timing-experiment bits; non-zero, the context says that results are not valid
	int dbg2 = al_env_int("AL_DBG2", 0);                                   // AL_DBG2: more of them; bit 5 (the shadow mode of the DP's early exit) keeps results valid
	bool dp_exit = al_env_int("AL_DP_EXIT", 1) != 0;                       // AL_DP_EXIT (on unless 0): the DP's early exit
	int dp_exit_stride = al_env_int("AL_DP_EXIT_STRIDE", 8);               // AL_DP_EXIT_STRIDE (1, 2, 4 or 8): the exit rule is evaluated every this-many anti-diagonals; anything else falls back to 8 ...
	const char *dp_exit_stride_refused = nullptr;                          // ... and this is the refused text, for the context's message
};
inline AlEnvCtx al_env_ctx()
{
	AlEnvCtx e;
	const int v = e.dp_exit_stride;
	if (v != 1 && v != 2 && v != 4 && v != 8) { e.dp_exit_stride = 8; e.dp_exit_stride_refused = getenv("AL_DP_EXIT_STRIDE"); }
	return e;
}

// ---- call: what the launcher or the system sets ----------------------------------------------------------------------------------------------------------
inline std::optional<int> al_env_rank() { return al_env_opt_int("RANK"); }
inline std::optional<int> al_env_world_size() { return al_env_opt_int("WORLD_SIZE"); }
// The device of a caller that names none (device < 0): LOCAL_RANK, else `fallback`, modulo the device count.
inline int al_env_pick_device(int device, int n_dev, int fallback = 0)
{
	if (device >= 0) return device;
	device = al_env_int("LOCAL_RANK", fallback);
	return n_dev > 0 ? device % n_dev : device;
}
// The id every rank of one launch shares: the first non-empty of AL_RUN_ID, TORCHELASTIC_RUN_ID and MASTER_PORT, or nullptr.
inline const char *al_env_run_id()
{
	for (const char *k : {"AL_RUN_ID", "TORCHELASTIC_RUN_ID", "MASTER_PORT"}) { const char *v = getenv(k); if (v && *v) return v; }
	return nullptr;
}
inline bool al_env_run_id_vouched() { return al_env_present("AL_RUN_ID"); }   // the second rule of AL_RUN_ID (present): the caller vouches for a fresh id, no token is agreed on
inline const char *al_env_tmpdir() { const char *td = getenv("TMPDIR"); return td && *td ? td : "/tmp"; }
// Set inside the process, so never cached: the CLI turns --sort-mem into AL_SORT_MEM and a missing -K into AL_AUTO_BATCH after its first look at the table,
// and the library's self-tests switch AL_NO_PWRITE and AL_RANK_BATCH between their cases.
inline uint64_t al_env_sort_mem() { return al_env_u64("AL_SORT_MEM", (uint64_t)16 << 30); }   // AL_SORT_MEM: bytes the sorted-BAM store holds in memory before it spills a run
inline bool al_env_auto_batch() { return al_env_present("AL_AUTO_BATCH"); }                    // AL_AUTO_BATCH (present): -K is no bound on a batch, the stream driver sizes it alone
inline bool al_env_no_pwrite() { return al_env_present("AL_NO_PWRITE"); }                      // AL_NO_PWRITE (present): ordered writes instead of pwrite at known offsets
inline long long al_env_rank_batch() { return al_env_ll("AL_RANK_BATCH", 0); }                 // AL_RANK_BATCH: records per grid batch of a multi-process run (<= 0: sized from the input)

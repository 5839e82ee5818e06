// al_devmem.h -- where device memory comes from (al_devmem.cpp): al_dev_malloc / al_dev_free and what sits behind them -- the AL_TEST_GUARD / AL_TEST_POISON
// fence, the per-owner accounting, the device memory reserve (its free list: al_range_pool.h) and the margin rule that leaves the runtime room.
// Not behind them (plain hipMalloc / hipFree on the product path, neither margin rule nor reserve; routing them here would change when they synchronise and
// when they are refused): al_sort_keys, al_winsrc_create, al_idx_cal_max_occ (al_index_dev.hip), al_batch_prefilter_decisions (al_prefilter.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <atomic>

// Set when a device allocation fails; al_batch_run reports AL_ERR_NOMEM then (the context stays usable: every DevBuf is
// either at its old size or empty, and the caller may upload a smaller batch).
inline bool &al_nomem_flag() { static thread_local bool f = false; return f; }

// Device ranges of the grow-only arenas and the index builder's temporaries, behind one pair of functions so that the test switches
// AL_TEST_POISON / AL_TEST_GUARD (al_devmem.cpp) see every range.  With a reserve (al_device_reserve: chunks obtained by a background thread) they are
// served from it, best fit, no driver call; without one, or for a request larger than a chunk, by hipMalloc / hipFree.
// al_dev_free does NOT synchronise the device (hipFree did): a range goes back to the reserve at once and may be handed to another context's thread in the
// next microsecond, so the caller frees a range only when no kernel or copy that uses it can still be in flight -- DevBuf::ensure(!keep) / release() are
// called between a context's batches, on the thread that has just synchronised its streams; ctx_release_buffers drains every stream first.
hipError_t al_dev_malloc(void **p, size_t bytes);
// Accounting: while a thread has set al_acct() to a counter, the bytes of every range it allocates are added to it (and taken off
// again when the range is freed, by whichever thread): the stream driver sizes its batches from what one batch held.
std::atomic<size_t> *&al_acct();
// time this process has spent in device / page-locked host allocation calls (AL_TIMING report)
struct AlAllocSite { const char *file; int line; };
AlAllocSite &al_alloc_site();      // who asked (AL_TRACE_ALLOC lists the large allocations with their call site)
struct AlAllocStat { std::atomic<long long> dev_ns{0}, dev_bytes{0}, dev_calls{0}, host_ns{0}, host_bytes{0}, host_calls{0}; };
AlAllocStat &al_alloc_stat();
void al_dev_free(void *p);
double al_long_batch_cap(double reads); // the stream driver's bound on a long input's batches (reads per batch) for an input of about `reads` reads: AL_LONG_BATCH, else 524 288, 2^20 from 200 M reads (al_devmem.cpp, beside the reserve's sizing, which restates the driver's rule)
long long al_dev_reserve_room();      // bytes the process's reserve still holds free (or is yet to obtain) on the current device; -1 = no reserve there
hipError_t al_dev_mem_info(size_t *free_b, size_t *total_b);   // hipMemGetInfo plus what the process's reserve (al_device_reserve) holds free
int al_dev_guard_check();            // AL_TEST_GUARD=1: number of live ranges whose guard zones were written (messages on stderr)

// al_devmem.cpp -- the device memory allocator (al_devmem.h): every device range of the product comes from al_dev_malloc / al_dev_free here.
// Host code, no kernels.  Four layers: the test fence (AL_TEST_GUARD / AL_TEST_POISON), the per-owner accounting, the device memory reserve
// (DevPool: a lock, a filler thread and the HIP calls around the free list of al_range_pool.h) and the margin rule of plain hipMalloc.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <sys/types.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <map>
#include <mutex>
#include <thread>
#include <vector>
#include "../../include/airlift.h"
#include "al_devmem.h"
#include "al_env.h"
#include "al_range_pool.h"

// Test switches of the allocator.  AL_TEST_POISON=<byte>: every new range is filled with that byte, so that a kernel that reads
// what nobody wrote shows up (the driver's fresh ranges are zero, which hides such reads);
// AL_TEST_POISON_ONLY=<n> restricts it to the n-th allocation of the process, AL_TEST_POISON_LOG prints sequence numbers and sizes.
// AL_TEST_GUARD=1: 4 KB of 0xCD on either side of every range, checked when the range is freed and by al_dev_guard_check():
// the driver pads ranges to pages, so a kernel that writes a few bytes past its buffer goes unnoticed otherwise.
static hipError_t al_dev_malloc_raw(void **p, size_t bytes);
static void al_dev_free_raw(void *p);
namespace { struct GuardRec { size_t bytes; int seq; }; std::mutex g_guard_m; std::map<void *, GuardRec> g_guard; std::atomic<int> g_alloc_seq(0); const size_t GUARD = 4096; }
static int guard_check_one(void *user, const GuardRec &r)
{
	std::vector<unsigned char> h(2 * GUARD);
	if (hipDeviceSynchronize() != hipSuccess) return 0;
	if (hipMemcpy(h.data(), (char *)user - GUARD, GUARD, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(h.data() + GUARD, (char *)user + r.bytes, GUARD, hipMemcpyDeviceToHost) != hipSuccess) return 0;
	int bad = 0;
	for (size_t i = 0; i < GUARD; ++i) if (h[i] != 0xCD) { fprintf(stderr, "[airlift] GUARD: alloc #%d (%zu bytes): byte %zd BEFORE the range overwritten (0x%02x)\n", r.seq, r.bytes, (ssize_t)i - (ssize_t)GUARD, h[i]); ++bad; break; }
	for (size_t i = 0; i < GUARD; ++i) if (h[GUARD + i] != 0xCD) { fprintf(stderr, "[airlift] GUARD: alloc #%d (%zu bytes): byte +%zu AFTER the range overwritten (0x%02x)\n", r.seq, r.bytes, i, h[GUARD + i]); ++bad; break; }
	return bad;
}
int al_dev_guard_check()
{
	std::lock_guard<std::mutex> l(g_guard_m);
	int bad = 0;
	for (auto &kv : g_guard) bad += guard_check_one(kv.first, kv.second);
	return bad;
}
hipError_t al_dev_malloc(void **p, size_t bytes)
{
	const char *const poison = al_env().test_poison, *const only = al_env().test_poison_only; const bool plog = al_env().test_poison_log, guard = al_env().test_guard;
	if (guard) {
		void *raw = nullptr;
		const hipError_t e = al_dev_malloc_raw(&raw, bytes + 2 * GUARD);
		if (e != hipSuccess) return e;
		const int n = g_alloc_seq.fetch_add(1);
		(void)hipMemset(raw, 0xCD, bytes + 2 * GUARD); (void)hipMemset((char *)raw + GUARD, poison ? atoi(poison) : 0, bytes); (void)hipDeviceSynchronize();
		*p = (char *)raw + GUARD;
		if (plog) fprintf(stderr, "[airlift] alloc #%d: %zu bytes\n", n, bytes);
		std::lock_guard<std::mutex> l(g_guard_m); g_guard[*p] = GuardRec{bytes, n};
		return hipSuccess;
	}
	const hipError_t e = al_dev_malloc_raw(p, bytes);
	if (e == hipSuccess && poison) {
		const int n = g_alloc_seq.fetch_add(1);
		if (plog) fprintf(stderr, "[airlift] alloc #%d: %zu bytes\n", n, bytes);
		if (!only || atoi(only) == n) { (void)hipMemset(*p, atoi(poison), bytes); (void)hipDeviceSynchronize(); }
	}
	return e;
}
void al_dev_free(void *p)
{
	if (!p) return;
	if (al_env().test_guard) {
		GuardRec r{0, -1}; bool found = false;
		{ std::lock_guard<std::mutex> l(g_guard_m); auto it = g_guard.find(p); if (it != g_guard.end()) { r = it->second; found = true; g_guard.erase(it); } }
		if (found) { (void)guard_check_one(p, r); al_dev_free_raw((char *)p - GUARD); return; }
	}
	al_dev_free_raw(p);
}
std::atomic<size_t> *&al_acct() { static thread_local std::atomic<size_t> *a = nullptr; return a; }
namespace { struct OwnRec { size_t bytes; std::atomic<size_t> *owner; }; std::mutex g_own_m; std::map<void *, OwnRec> g_own; }
AlAllocStat &al_alloc_stat() { static AlAllocStat s; return s; }
AlAllocSite &al_alloc_site() { static thread_local AlAllocSite s{"", 0}; return s; }
// ---- device memory reserve (round 5) ----------------------------------------------------------------------------------------------------
// What a process pays for device memory on this platform is the driver mapping (and scrubbing) it: tenths of a second to seconds per 100 GB, inside
// the first batches of a file-to-file run.  al_device_reserve() starts a thread that obtains the run's memory in a few large chunks WHILE the
// reference is loaded and the index is built; al_dev_malloc / al_dev_free then serve every range -- index arrays, the index builder's temporaries,
// the contexts' grow-only workspaces, the slots' text buffers -- from those chunks (best fit, neighbours coalesced), without a driver call.
// A request that finds no room waits for the filler while it is still at work and falls back to hipMalloc otherwise (also: other devices, ranges
// larger than a chunk).  Peak use is reported (AL_TIMING) -- the workspace figure of the run.
namespace {
struct DevPool {
	int device = -1; std::mutex m; std::condition_variable cv;
	AlRangePool ranges;                                           // chunks, free and used blocks, in_use / peak / n_served: under m
	bool filling = false, started = false; size_t target = 0, obtained = 0, chunk = 0, n_missed = 0; double t_fill = 0, t_first = 0;
	std::thread filler;
	bool here() const { int dev = -1; return started && hipGetDevice(&dev) == hipSuccess && dev == device; }   // a reserve, and on the current device
};
DevPool &pool() { static DevPool *P = new DevPool(); return *P; }   // (never destroyed: the filler may outlive main())
void *pool_alloc(size_t bytes)
{
	DevPool &P = pool();
	if (!P.here() || bytes == 0) return nullptr;                   // (an empty request is the driver's, as without a reserve: the free list never serves one, and it must not wait for the filler)
	const size_t need = AlRangePool::round_up(bytes);
	std::unique_lock<std::mutex> l(P.m);
	for (;;) {
		if (const uintptr_t p = P.ranges.alloc(bytes)) return (void *)p;
		if (!P.filling || need > P.chunk) { ++P.n_missed; return nullptr; }
		P.cv.wait(l);
	}
}
bool pool_free(void *ptr)
{
	DevPool &P = pool();
	if (!P.started) return false;
	std::lock_guard<std::mutex> l(P.m);
	return P.ranges.free((uintptr_t)ptr);
}
// chunks nothing is using go back to the driver (and the filler stops): the request that did not fit the reserve gets a chance at hipMalloc
size_t pool_release_free(void)
{
	DevPool &P = pool();
	if (!P.started) return 0;
	std::vector<uintptr_t> rel; size_t bytes = 0;
	{
		std::lock_guard<std::mutex> l(P.m);
		bytes = P.ranges.take_unused_chunks(rel);
		P.obtained -= bytes; P.target = P.obtained;                  // (the filler asks for no further chunk)
	}
	for (uintptr_t q : rel) (void)hipFree((void *)q);
	if (bytes && al_env().timing) fprintf(stderr, "[airlift] device memory reserve: %.1f GB in %zu unused chunk(s) given back to the driver for a request the reserve could not serve\n", bytes / 1e9, rel.size());
	return bytes;
}
}
extern "C" int al_device_reserve(int device, uint64_t bytes)
{
	DevPool &P = pool();
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return -1;
	device = al_env_pick_device(device, n_dev);
	if (device >= n_dev || bytes == 0) return -1;
	{
		std::lock_guard<std::mutex> l(P.m);
		if (P.started) return P.device == device ? 0 : -1;          // one reserve per process
		size_t free_b = 0, total_b = 0;
		if (hipSetDevice(device) != hipSuccess || hipMemGetInfo(&free_b, &total_b) != hipSuccess) return -1;
		P.device = device; P.target = (size_t)std::min<uint64_t>(bytes, (uint64_t)((double)free_b * 0.92));
		const double chunk_gb = al_env().pool_chunk_gb;
		P.chunk = chunk_gb > 0 ? (size_t)(chunk_gb * 1e9) : std::min<size_t>(std::max<size_t>(P.target / 6, (size_t)2 << 30), (size_t)24 << 30);
		P.chunk = P.chunk / AlRangePool::ALIGN * AlRangePool::ALIGN;
		P.started = true; P.filling = true;
	}
	P.filler = std::thread([&P]() {
		const auto t0 = std::chrono::steady_clock::now();
		(void)hipSetDevice(P.device);
		for (;;) {
			size_t want;
			{ std::lock_guard<std::mutex> l(P.m); want = P.target > P.obtained ? std::min(P.chunk, P.target - P.obtained) : 0; }
			if (want < ((size_t)64 << 20)) break;
			void *p = nullptr;
			if (hipMalloc(&p, want) != hipSuccess) { (void)hipGetLastError(); break; }
			std::lock_guard<std::mutex> l(P.m);
			P.ranges.add_chunk((uintptr_t)p, want); P.obtained += want;
			if (P.ranges.regions.size() == 1) P.t_first = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
			P.cv.notify_all();
		}
		std::lock_guard<std::mutex> l(P.m);
		P.filling = false; P.t_fill = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
		P.cv.notify_all();
	});
	P.filler.detach();
	return 0;
}
// Reads per batch of a long input.  Measured on 12.5 M reads of C4 (round 6): batches of 2^20 reads map 11.7 M reads/s against 10.95 M with 524 288 (a batch's serial tails weigh
// half as much), but the run then holds 183 GB instead of 106 GB, and what a process asks for beyond ~128 GB the driver hands out at 35 - 70 GB/s (it clears the pages): start-up
// + 1.5 ... 2.9 s, whole process 2.7 -> 4.9 - 5.3 s.  So the large batch is for inputs whose pipeline runs long enough to pay for that: from AL_LONG_BATCH_BIG_FROM reads
// (default 200 M: ~20 s of pipeline, 7 % of which is 1.4 s).
double al_long_batch_cap(double reads)
{
	const double fixed = al_env().long_batch, big_from = al_env().long_batch_big_from;
	return fixed > 0 ? fixed : reads >= big_from ? 1048576.0 : 524288.0;
}
// The reserve a file-to-file run needs, from its file sizes alone (the stream driver's own arithmetic, al_stream_pipe.cpp: ~360 bytes of FASTQ per
// read; inputs of >= 3 M reads run 2 contexts x 524288-read batches, shorter ones 3 x 131072): the index (4-bit sequence, 8 bytes per minimizer
// occurrence at one minimizer per ~5.7 bases, a table of 16-byte entries at load <= 0.5) + the larger of the index builder's temporaries and the
// contexts' workspaces + the slots' text.  Workspace bytes per read of a batch follow the reference's size -- seed hits per read grow with its repeat
// content: ~78 KB per read measured on a 3.1 Gbp reference with 45 % repeats, ~5 KB on a yeast-sized one; AL_RESERVE_KB_PER_READ overrides.
extern "C" int64_t al_device_reserve_for_run(int device, const char *ref_fn, int n_fn, const char *const *fn)
{
	if (al_env().no_reserve) return 0;
	struct stat sb;
	if (!ref_fn || stat(ref_fn, &sb) != 0 || !S_ISREG(sb.st_mode)) return 0;
	const double G = (double)sb.st_size;
	double fq = 0;
	for (int i = 0; i < n_fn; ++i) { if (!fn[i] || stat(fn[i], &sb) != 0 || !S_ISREG(sb.st_mode)) return 0; const size_t L = strlen(fn[i]); if (L > 3 && !strcmp(fn[i] + L - 3, ".gz")) return 0; fq += (double)sb.st_size; }
	const double reads = fq / 360.0;
	if (reads < 2.0e5) return 0;                                   // a short run: the driver's own pace is no issue
	const double n_min = G / 5.7;
	double tab = 32.0; while (tab < 2.0 * 0.9 * n_min + 2.0) tab *= 2.0; tab *= 16.0;
	const double index = 0.5 * G + 8.0 * n_min + tab, build_tmp = G + 4.0 * 8.0 * n_min + 4.0 * n_min;
	const double kb = al_env().reserve_kb_per_read.value_or(G >= 1.0e9 ? 85.0 : G >= 2.0e8 ? 40.0 : 12.0);
	const bool long_input = reads >= 3.0e6;
	// (a long input's batch by the stream driver's own rule: at least three batches per context)
	const double batch = long_input ? std::min(al_long_batch_cap(reads), std::max(262144.0, reads / 6.0)) : std::min(131072.0, reads), n_ctx = long_input ? 2.0 : 3.0, n_slots = long_input ? 4.0 : 5.0;
	const double ws = n_ctx * batch * kb * 1024.0 + n_slots * batch * 2300.0 + 1.5e9;
	const double need = index + std::max(build_tmp, ws) * 1.08;
	if (al_device_reserve(device, (uint64_t)need) != 0) return -1;
	return (int64_t)need;
}
// free / total device memory as the batch sizing sees it: what the driver reports plus what the reserve holds free
// (memory the filler has yet to obtain is already part of the driver's free figure)
hipError_t al_dev_mem_info(size_t *free_b, size_t *total_b)
{
	const hipError_t e = hipMemGetInfo(free_b, total_b);
	DevPool &P = pool();
	if (e == hipSuccess && P.here()) { std::lock_guard<std::mutex> l(P.m); *free_b += P.ranges.free_bytes(); }
	return e;
}
// bytes the reserve holds free on the current device (and still has to obtain); -1 without a reserve there
long long al_dev_reserve_room()
{
	DevPool &P = pool();
	if (!P.here()) return -1;
	std::lock_guard<std::mutex> l(P.m);
	return (long long)(P.ranges.free_bytes() + (P.filling && P.target > P.obtained ? P.target - P.obtained : 0));
}
extern "C" void al_device_reserve_report(FILE *fp)
{
	DevPool &P = pool();
	if (!P.started) return;
	std::lock_guard<std::mutex> l(P.m);
	fprintf(fp, "[airlift] device memory reserve: %.1f of %.1f GB obtained in %zu chunk(s) of %.1f GB by the background thread in %.3f s%s (first chunk after %.3f s); peak in use %.2f GB, %zu ranges served, %zu requests passed on to hipMalloc\n",
	        P.obtained / 1e9, P.target / 1e9, P.ranges.regions.size(), P.chunk / 1e9, P.t_fill, P.filling ? " (still filling)" : "", P.t_first, P.ranges.peak / 1e9, P.ranges.n_served, P.n_missed);
}
extern "C" uint64_t al_device_reserve_peak(void) { DevPool &P = pool(); if (!P.started) return 0; std::lock_guard<std::mutex> l(P.m); return (uint64_t)P.ranges.peak; }
extern "C" void al_device_reserve_reset_peak(void) { DevPool &P = pool(); if (!P.started) return; std::lock_guard<std::mutex> l(P.m); P.ranges.reset_peak(); }

// hipMalloc that leaves the runtime room (round 6).  The HIP runtime obtains device memory of its own while kernels run -- the scratch of a hardware queue the
// first time a kernel with private memory is dispatched on it (k_align: 272 bytes per lane, x 64 lanes x the wave slots of 256 CUs = 142 MB per queue, and a
// context spreads its streams over up to 16 queues), code objects, signals -- and when it cannot, the process dies with HSA_STATUS_ERROR_OUT_OF_RESOURCES: no
// error a caller can catch.  So a request that would leave less than a margin free is refused HERE, as out of memory (AL_ERR_NOMEM upstream: the drivers halve
// the batch).  AL_HBM_MARGIN_MB, default 2048.  With a reserve, its free chunks go back to the driver first and the request is tried again -- also for a request
// larger than a chunk, which the reserve can never serve itself.
static hipError_t al_hip_malloc_margin(void **p, size_t bytes)
{
	const size_t margin = (size_t)al_env().hbm_margin_mb << 20;
	for (int attempt = 0; attempt < 2; ++attempt) {
		size_t fr = 0, tot = 0;
		const bool known = hipMemGetInfo(&fr, &tot) == hipSuccess;
		if (!known) (void)hipGetLastError();
		if (!known || fr >= bytes + margin) {
			const hipError_t e = hipMalloc(p, bytes);
			if (e == hipSuccess) return e;
			(void)hipGetLastError();
		}
		if (attempt == 0 && pool_release_free() == 0) break;
	}
	*p = nullptr;
	return hipErrorOutOfMemory;
}
static hipError_t al_dev_malloc_raw(void **p, size_t bytes)
{
	const auto t0 = std::chrono::steady_clock::now();
	hipError_t e = hipSuccess;
	if (void *q = pool_alloc(bytes)) *p = q; else e = al_hip_malloc_margin(p, bytes);
	{ AlAllocStat &a = al_alloc_stat(); const long long ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); a.dev_ns += ns; a.dev_bytes += (long long)bytes; ++a.dev_calls;
	  if (al_env().trace_alloc && bytes >= (32u << 20)) { const AlAllocSite &w = al_alloc_site(); const char *b = strrchr(w.file, '/'); fprintf(stderr, "[airlift] alloc: %8.1f MB in %7.1f ms for %s:%d\n", bytes / 1e6, ns / 1e6, b ? b + 1 : w.file, w.line); } }
	al_alloc_site() = AlAllocSite{"", 0};
	std::atomic<size_t> *a = al_acct();
	if (e == hipSuccess && a) { a->fetch_add(bytes); std::lock_guard<std::mutex> l(g_own_m); g_own[*p] = OwnRec{bytes, a}; }
	return e;
}
static void al_dev_free_raw(void *p)
{
	if (!p) return;
	{ std::lock_guard<std::mutex> l(g_own_m); auto it = g_own.find(p); if (it != g_own.end()) { it->second.owner->fetch_sub(it->second.bytes); g_own.erase(it); } }
	const auto t0 = std::chrono::steady_clock::now();
	if (!pool_free(p)) (void)hipFree(p);
	al_alloc_stat().dev_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
}

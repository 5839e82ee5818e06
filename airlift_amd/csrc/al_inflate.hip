// al_inflate.hip -- BGZF members inflated on the GPU (--gpu-inflate; product code).  The function computed is the one written down at the head of
// al_dev_inflate.h; this file is its evaluation by a wavefront per member, the device backend, and the reader AlBgzfIn (al_bam.h) that drives it.
//
// k_inflate: a persistent grid of workgroups of four wavefronts; a wavefront takes the next member off a counter until the list is empty.  Lane 0 runs
// the token decoder (al_inf_next: bit reader, Huffman tables in the wavefront's 2.7 KB of LDS, every validity and bounds check) and leaves up to 64
// tokens in LDS; the 64 lanes then place them: the tokens' output offsets are a prefix sum over the lanes, every literal is one lane's store, and the
// matches and stored runs are copied one after the other by all lanes (a match shorter than its distance reads distinct earlier bytes; one that
// overlaps itself reads out[start - dist + j % dist], which lies before the match as well).  Back-references read the member's own earlier output in
// global memory; a wavefront's memory operations complete in order, and a fence stands between the stores of one step and the loads of the next.
// There is no workgroup barrier anywhere: the four wavefronts of a workgroup share nothing but the launch.  CRC32 of the ISIZE bytes is computed by
// the same wavefront right after (64 byte ranges, joined pairwise as in k_deflate), so a member's status is final when the kernel ends.
//
// AlBgzfIn: a producer thread reads pieces of the file, lists whole members along the BSIZE chain (a cut member is carried), sends the piece up,
// launches k_inflate and brings the bytes down, alternating between two streams so that the copies of one piece overlap the kernel of the next; read()
// consumes the pieces in file order.  Without device memory (or a device) the pieces are inflated by zlib, member by member, on worker threads.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fcntl.h>
#include <unistd.h>
#include <zlib.h>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "al_runtime.h"
#include "al_io.h"
#include "al_bam.h"
#include "al_dev_inflate.h"

namespace {

const uint32_t INF_T = 256, INF_WAVES = INF_T / 64, INF_BATCH = 64;

struct InfWaveLds { AlInfTab T; uint32_t a[INF_BATCH], b[INF_BATCH], ctl[4]; };

// orders a wavefront's stores before its later loads (they complete in order; this keeps the compiler from moving them) and its LDS traffic likewise
__device__ __forceinline__ void inf_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __builtin_amdgcn_wave_barrier(); }

// in: the piece's bytes; mem[0, n_mem): the members (in_off into `in`, out_off into `out`); status[m]: 0 or AL_INF_E_*; *next: 0 at launch.
__global__ __launch_bounds__(256) void k_inflate(const uint8_t *in, const AlInfMember *mem, uint32_t n_mem, uint8_t *out, uint32_t *status, uint32_t *next)
{
	__shared__ InfWaveLds lds[INF_WAVES];
	const uint32_t lane = threadIdx.x & 63;
	InfWaveLds &L = lds[threadIdx.x >> 6];
	for (;;) {
		uint32_t mi = 0;
		if (lane == 0) mi = atomicAdd(next, 1u);
		mi = (uint32_t)__shfl((int)mi, 0, 64);
		if (mi >= n_mem) break;
		const AlInfMember M = mem[mi];
		const uint8_t *m = in + M.in_off; uint8_t *o = out + M.out_off;
		uint32_t ms = 0, hdr = 0;
		if (al_inf_parse_header(m, M.msize, &ms, &hdr) != 0 || ms != M.msize || M.isize > AL_INF_MAX_ISIZE) { if (lane == 0) status[mi] = AL_INF_E_HEADER; continue; }
		const uint8_t *ds = m + hdr;
		AlInfState s; al_inf_init(s, ds, M.msize - hdr - 8, M.isize);
		uint32_t base = 0;
		for (;;) {          // a round hands out at least one token or ends the member: at most ISIZE + 1 rounds
			if (lane == 0) {
				uint32_t n = 0, a = 0, b = 0, ended = 0;
				while (n < INF_BATCH) {
					if (!al_inf_next(s, &L.T, &a, &b)) { ended = 1; break; }
					L.a[n] = a; L.b[n] = b; ++n;
					if ((a & 0xc0000000u) == AL_INF_TOK_STORED) break;
				}
				L.ctl[0] = n; L.ctl[1] = ended;
			}
			inf_fence();
			const uint32_t n = L.ctl[0], ended = L.ctl[1];
			const uint32_t a = lane < n ? L.a[lane] : 0, b = lane < n ? L.b[lane] : 0;
			const bool run = lane < n && (a & 0xc0000000u) != 0;
			const uint32_t mylen = lane >= n ? 0 : (a & AL_INF_TOK_MATCH) ? (a >> 16 & 0x1ff) : (a & AL_INF_TOK_STORED) ? (a & 0xffff) : 1;
			uint32_t x = mylen;
			for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)x, d, 64); if (lane >= d) x += y; }
			const uint32_t off = base + x - mylen;                       // (al_inf_next has checked base + x <= ISIZE for every token it handed out)
			base += (uint32_t)__shfl((int)x, 63, 64);
			if (lane < n && !run) o[off] = (uint8_t)a;
			uint64_t todo = __ballot(run);
			while (todo) {
				const int k = __builtin_ctzll(todo); todo &= todo - 1;
				const uint32_t ka = (uint32_t)__shfl((int)a, k, 64), kb = (uint32_t)__shfl((int)b, k, 64), ko = (uint32_t)__shfl((int)off, k, 64);
				inf_fence();
				if (ka & AL_INF_TOK_MATCH) {
					const uint32_t len = ka >> 16 & 0x1ff, dist = (ka & 0xffff) + 1;       // dist <= ko: checked by al_inf_next
					const uint8_t *src = o + (ko - dist);
					for (uint32_t j = lane; j < len; j += 64) o[ko + j] = src[dist >= len ? j : j % dist];
				} else {
					const uint32_t len = ka & 0xffff;                                      // kb + len <= csize: checked by al_inf_next
					for (uint32_t j = lane; j < len; j += 64) o[ko + j] = ds[kb + j];
				}
			}
			inf_fence();
			if (ended) break;
		}
		int st = lane == 0 ? al_inf_finish(s) : 0;
		st = __shfl(st, 0, 64);
		if (st == 0) {
			uint32_t crc = 0;
			if (M.isize) {      // the bytes right-aligned in 64 ranges of c, a range per lane, the registers joined pairwise
				const uint32_t c = (M.isize + 63) / 64, pad = 64 * c - M.isize;
				uint32_t r = 0;
				for (uint32_t k = 0; k < c; ++k) { const uint32_t v = lane * c + k; if (v < pad) continue; const uint32_t i = v - pad; if (i == 0) r = 0xffffffffu; r = al_dfl_crc_byte(r, o[i]); }
				uint32_t xp = al_dfl_crc_xpow8(c);
				for (uint32_t w = 1; w < 64; w <<= 1) {
					const uint32_t other = (uint32_t)__shfl_down((int)r, w, 64);
					if ((lane & (2 * w - 1)) == 0) r = al_dfl_crc_mul(r, xp) ^ other;
					xp = al_dfl_crc_mul(xp, xp);
				}
				crc = ~(uint32_t)__shfl((int)r, 0, 64);
			}
			if (crc != al_inf_le32(m + M.msize - 8)) st = AL_INF_E_CRC;
		}
		if (lane == 0) status[mi] = (uint32_t)st;
	}
}

} // namespace
// the launch alone, for a caller with buffers of its own (the stream driver's slots, al_stream.hip): n_mem > 0 members of d_in to d_out, *d_next zero;
// cu4 = 4 x the device's compute units.  0, or -1 when the launch failed
int al_inflate_launch(hipStream_t st, int cu4, const uint8_t *d_in, const AlInfMember *d_mem, uint32_t n_mem, uint8_t *d_out, uint32_t *d_status, uint32_t *d_next)
{
	const uint32_t grid = (uint32_t)std::min<size_t>(((size_t)n_mem + INF_WAVES - 1) / INF_WAVES, (size_t)cu4);
	hipLaunchKernelGGL(k_inflate, dim3(grid), dim3(INF_T), 0, st, d_in, d_mem, n_mem, d_out, d_status, d_next);
	return hipGetLastError() == hipSuccess ? 0 : -1;
}
namespace {

inline double inf_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// one queue of the device backend: a stream, its device buffers and the events around its three steps
struct InfQueue {
	hipStream_t st = nullptr; hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
	uint8_t *d_in = nullptr, *d_out = nullptr; AlInfMember *d_mem = nullptr; uint32_t *d_status = nullptr, *d_next = nullptr;
};
struct InfDev {
	int device = 0, grid = 0; bool open = false; InfQueue q[2];
};
void inf_dev_close(InfDev &d)
{
	if (!d.open) return;
	(void)hipSetDevice(d.device);
	for (InfQueue &q : d.q) {
		if (q.st) (void)hipStreamSynchronize(q.st);
		if (q.d_in) al_dev_free(q.d_in); if (q.d_out) al_dev_free(q.d_out); if (q.d_mem) al_dev_free(q.d_mem); if (q.d_status) al_dev_free(q.d_status); if (q.d_next) al_dev_free(q.d_next);
		for (hipEvent_t &e : q.ev) if (e) (void)hipEventDestroy(e);
		if (q.st) (void)hipStreamDestroy(q.st);
		q = InfQueue();
	}
	d.open = false;
}
// 0: open with room for pieces of cap_in bytes, cap_out inflated bytes, cap_mem members on n_q queues; 1: the device refused the memory; -1: no usable device
int inf_dev_open(InfDev &d, int device, size_t cap_in, size_t cap_out, size_t cap_mem, int n_q)
{
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) { (void)hipGetLastError(); return -1; }
	device = al_env_pick_device(device, n_dev);
	hipDeviceProp_t pr;
	if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&pr, device) != hipSuccess) { (void)hipGetLastError(); return -1; }
	d.device = device; d.open = true;
	d.grid = (pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 64) * 4;
	const bool refuse = al_env().test_inflate_nomem;          // (test switch, DESIGN.md section 8: every request is refused)
	for (int i = 0; i < n_q; ++i) {
		InfQueue &q = d.q[i];
		if (hipStreamCreateWithFlags(&q.st, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); inf_dev_close(d); return -1; }
		for (hipEvent_t &e : q.ev) if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); inf_dev_close(d); return -1; }
		bool ok = !refuse;
		ok = ok && al_dev_malloc((void **)&q.d_in, cap_in) == hipSuccess;
		ok = ok && al_dev_malloc((void **)&q.d_out, cap_out) == hipSuccess;
		ok = ok && al_dev_malloc((void **)&q.d_mem, cap_mem * sizeof(AlInfMember)) == hipSuccess;
		ok = ok && al_dev_malloc((void **)&q.d_status, cap_mem * 4) == hipSuccess;
		ok = ok && al_dev_malloc((void **)&q.d_next, 4) == hipSuccess;
		if (!ok) { (void)hipGetLastError(); inf_dev_close(d); return 1; }
	}
	return 0;
}
// a piece on queue q, all of it asynchronous: n_in bytes and n_mem members up, the kernel, n_out bytes and the status words down (host buffers page-locked)
bool inf_dev_enqueue(InfDev &d, int qi, const uint8_t *h_in, size_t n_in, const AlInfMember *h_mem, size_t n_mem, uint8_t *h_out, size_t n_out, uint32_t *h_status, uint8_t *d_out_at = nullptr)
{
	InfQueue &q = d.q[qi];
	uint8_t *d_out = d_out_at ? d_out_at : q.d_out;
	bool ok = hipEventRecord(q.ev[0], q.st) == hipSuccess;
	ok = ok && hipMemcpyAsync(q.d_in, h_in, n_in, hipMemcpyHostToDevice, q.st) == hipSuccess;
	ok = ok && hipMemcpyAsync(q.d_mem, h_mem, n_mem * sizeof(AlInfMember), hipMemcpyHostToDevice, q.st) == hipSuccess;
	ok = ok && hipMemsetAsync(q.d_next, 0, 4, q.st) == hipSuccess;
	ok = ok && hipEventRecord(q.ev[1], q.st) == hipSuccess;
	if (ok) { ok = al_inflate_launch(q.st, d.grid, q.d_in, q.d_mem, (uint32_t)n_mem, d_out, q.d_status, q.d_next) == 0; }
	ok = ok && hipEventRecord(q.ev[2], q.st) == hipSuccess;
	ok = ok && (n_out == 0 || hipMemcpyAsync(h_out, d_out, n_out, hipMemcpyDeviceToHost, q.st) == hipSuccess);
	ok = ok && hipMemcpyAsync(h_status, q.d_status, n_mem * 4, hipMemcpyDeviceToHost, q.st) == hipSuccess;
	ok = ok && hipEventRecord(q.ev[3], q.st) == hipSuccess;
	return ok;
}
bool inf_dev_wait(InfDev &d, int qi, double *h2d_s, double *kernel_s, double *d2h_s)
{
	InfQueue &q = d.q[qi];
	if (hipStreamSynchronize(q.st) != hipSuccess) return false;
	float ms = 0;
	if (hipEventElapsedTime(&ms, q.ev[0], q.ev[1]) == hipSuccess && h2d_s) *h2d_s += ms * 1e-3;
	if (hipEventElapsedTime(&ms, q.ev[1], q.ev[2]) == hipSuccess && kernel_s) *kernel_s += ms * 1e-3;
	if (hipEventElapsedTime(&ms, q.ev[2], q.ev[3]) == hipSuccess && d2h_s) *d2h_s += ms * 1e-3;
	return true;
}

// the host backend: members [0, n_mem) of buf inflated by zlib into out, CRC32 checked, on n_threads workers; a member zlib turns down gets its status from the twin
void inf_host_run(const uint8_t *buf, const AlInfMember *mem, size_t n_mem, uint8_t *out, uint32_t *status, int n_threads, double *inflate_s, double *crc_s)
{
	const double t0 = inf_now();
	al_parallel_for(n_threads > 1 ? n_threads : 1, n_mem, [&](size_t lo, size_t hi, int) {
		z_stream zs; memset(&zs, 0, sizeof(zs));
		const bool have = inflateInit2(&zs, -15) == Z_OK;
		for (size_t k = lo; k < hi; ++k) {
			const AlInfMember &M = mem[k]; const uint8_t *m = buf + M.in_off;
			uint32_t ms = 0, hdr = 0; bool good = false;
			if (have && al_inf_parse_header(m, M.msize, &ms, &hdr) == 0 && ms == M.msize) {
				inflateReset(&zs);
				Bytef dummy = 0;
				zs.next_in = (Bytef *)(m + hdr); zs.avail_in = M.msize - hdr - 8; zs.next_out = M.isize ? out + M.out_off : &dummy; zs.avail_out = M.isize;
				good = inflate(&zs, Z_FINISH) == Z_STREAM_END && zs.avail_in == 0 && zs.avail_out == 0;
			}
			status[k] = good ? 0u : 0x100u;
		}
		if (have) inflateEnd(&zs);
	});
	const double t1 = inf_now();
	al_parallel_for(n_threads > 1 ? n_threads : 1, n_mem, [&](size_t lo, size_t hi, int) {
		for (size_t k = lo; k < hi; ++k) {
			const AlInfMember &M = mem[k]; const uint8_t *m = buf + M.in_off;
			if (status[k] == 0) { if ((uint32_t)crc32(crc32(0L, Z_NULL, 0), out + M.out_off, M.isize) != al_inf_le32(m + M.msize - 8)) status[k] = AL_INF_E_CRC; continue; }
			std::vector<uint8_t> tmp(M.isize + 1);
			const int st = al_inflate_member_host(m, M.msize, tmp.data());
			status[k] = st ? (uint32_t)st : (uint32_t)AL_INF_E_SYMBOL;
		}
	});
	if (inflate_s) *inflate_s += t1 - t0;
	if (crc_s) *crc_s += inf_now() - t1;
}

} // namespace

// ---- the reader ---------------------------------------------------------------------------------------------------------------------------------------------
struct AlBgzfInImpl {
	enum { N_SLOT = 3 };
	struct Slot {
		uint8_t *h_in = nullptr, *h_out = nullptr; AlInfMember *h_mem = nullptr; uint32_t *h_status = nullptr;
		size_t n_in = 0, n_out = 0, n_mem = 0; uint64_t file_off = 0; int state = 0;      // 0: free, 1: being filled or in flight, 2: ready
		bool on_dev = false;
	};
	int fd = -1; uint64_t fpos = 0; bool eof = false;
	size_t piece = 0, cap_in = 0, cap_out = 0, cap_mem = 0;
	Slot slot[N_SLOT]; bool pinned = false;
	InfDev dev; bool use_dev = false; int n_threads = 1;
	std::vector<uint8_t> carry;
	std::thread th; std::mutex mu; std::condition_variable cv;
	uint64_t n_made = 0; bool done = false, stop = false;                                // pieces handed over; the producer has ended; the consumer has
	int err = 0; std::string msg; uint64_t err_piece = ~0ull;                           // the first piece that holds an error: read() fails when it gets there
	uint64_t k_cons = 0; bool have_cur = false; size_t beg = 0, end = 0;
	// AL_TIMING
	double t_read = 0, t_h2d = 0, t_kernel = 0, t_d2h = 0, t_crc = 0, t_host = 0, t_wait = 0; uint64_t n_members = 0, b_in = 0, b_out = 0, n_fallback = 0, n_pieces = 0;

	void fail(uint64_t k, const std::string &m) { std::lock_guard<std::mutex> g(mu); if (err == 0) { err = -2; msg = m; err_piece = k; } }
	// the next piece into slot s: carry + new bytes, members listed.  1: there is a piece; 0: the file has ended cleanly; -1: error (told through fail)
	int prepare(Slot &s, uint64_t k)
	{
		size_t n = carry.size();
		if (n) memcpy(s.h_in, carry.data(), n);
		s.file_off = fpos - n;
		std::vector<AlInfMember> mem;
		uint64_t pos = 0, out_n = 0; int lr = 0;
		for (;;) {
			if (!eof) {
				const double t0 = inf_now();
				size_t want = std::min(piece, cap_in - n);
				while (want) {
					const ssize_t g = pread(fd, s.h_in + n, want, (off_t)fpos);
					if (g < 0) { fail(k, "read error"); return -1; }
					if (g == 0) { eof = true; break; }
					n += (size_t)g; fpos += (uint64_t)g; want -= (size_t)g;
				}
				t_read += inf_now() - t0;
			}
			lr = al_inf_list(s.h_in, n, &pos, &out_n, cap_out, cap_mem, mem);
			if (lr == 0 && mem.empty() && !eof && n < cap_in) continue;
			break;
		}
		if (mem.empty()) {
			if (lr == 0 && n == 0) return 0;
			char t[160];
			snprintf(t, sizeof(t), lr ? "no BGZF member at file offset %llu" : "truncated BGZF member at file offset %llu", (unsigned long long)s.file_off);
			fail(k, t); return -1;
		}
		carry.assign(s.h_in + pos, s.h_in + n);
		memcpy(s.h_mem, mem.data(), mem.size() * sizeof(AlInfMember));
		s.n_in = (size_t)pos; s.n_out = (size_t)out_n; s.n_mem = mem.size();
		n_members += s.n_mem; b_in += s.n_in; b_out += s.n_out; ++n_pieces;
		return 1;
	}
	void check(Slot &s, uint64_t k)
	{
		for (size_t i = 0; i < s.n_mem; ++i) if (s.h_status[i]) {
			char t[200];
			snprintf(t, sizeof(t), "BGZF member at file offset %llu: status %u (%s)", (unsigned long long)(s.file_off + s.h_mem[i].in_off), s.h_status[i], al_inf_strerror((int)s.h_status[i]));
			fail(k, t); break;
		}
	}
	void hand_over(Slot &s) { { std::lock_guard<std::mutex> g(mu); s.state = 2; ++n_made; } cv.notify_all(); }
	void run()
	{
		if (use_dev) (void)hipSetDevice(dev.device);
		long prev = -1; uint64_t prev_k = 0;
		auto finish_prev = [&]() {
			if (prev < 0) return;
			Slot &p = slot[prev];
			if (!inf_dev_wait(dev, (int)(prev_k & 1), &t_h2d, &t_kernel, &t_d2h)) fail(prev_k, "the device inflater failed"); else check(p, prev_k);
			hand_over(p); prev = -1;
		};
		for (uint64_t k = 0;; ++k) {
			Slot &s = slot[k % N_SLOT];
			{ std::unique_lock<std::mutex> g(mu); cv.wait(g, [&] { return s.state == 0 || stop; }); if (stop) break; s.state = 1; }
			const int r = prepare(s, k);
			if (r <= 0) { finish_prev(); { std::lock_guard<std::mutex> g(mu); s.state = 0; } break; }
			if (use_dev) {
				if (!inf_dev_enqueue(dev, (int)(k & 1), s.h_in, s.n_in, s.h_mem, s.n_mem, s.h_out, s.n_out, s.h_status)) { finish_prev(); fail(k, "the device inflater failed"); hand_over(s); break; }
				finish_prev();
				prev = (long)(k % N_SLOT); prev_k = k;
			} else {
				inf_host_run(s.h_in, s.h_mem, s.n_mem, s.h_out, s.h_status, n_threads, &t_host, &t_crc);
				check(s, k); hand_over(s);
			}
			{ std::lock_guard<std::mutex> g(mu); if (err) break; }      // (a piece with a bad member was handed over: nothing behind it is wanted)
		}
		finish_prev();
		{ std::lock_guard<std::mutex> g(mu); done = true; }
		cv.notify_all();
	}
	void release()
	{
		if (th.joinable()) { { std::lock_guard<std::mutex> g(mu); stop = true; } cv.notify_all(); th.join(); }
		if (use_dev || dev.open) { inf_dev_close(dev); }
		for (Slot &s : slot) {
			if (pinned) { if (s.h_in) (void)hipHostFree(s.h_in); if (s.h_out) (void)hipHostFree(s.h_out); if (s.h_mem) (void)hipHostFree(s.h_mem); if (s.h_status) (void)hipHostFree(s.h_status); }
			else { free(s.h_in); free(s.h_out); free(s.h_mem); free(s.h_status); }
			s = Slot();
		}
		if (fd >= 0) close(fd);
		fd = -1;
	}
};

AlBgzfIn::AlBgzfIn(int dev, int nt) : device(dev), n_threads(nt > 1 ? nt : 1) {}
AlBgzfIn::~AlBgzfIn() { close(); }
void AlBgzfIn::close() { if (p) { p->release(); delete p; p = nullptr; } }
bool AlBgzfIn::failed() const { if (!p) return false; std::lock_guard<std::mutex> g(p->mu); return p->err != 0 && p->k_cons >= p->err_piece; }
const char *AlBgzfIn::message() const { return p ? p->msg.c_str() : ""; }

bool AlBgzfIn::open(const char *fn)
{
	plain = false;
	if (strcmp(fn, "-") == 0) { plain = true; return false; }
	const int fd = ::open(fn, O_RDONLY);
	if (fd < 0) return false;
	{   // BGZF?  (a gzip file without the BC subfield is read as one stream by the caller)
		uint8_t h[4096]; const ssize_t g = pread(fd, h, sizeof(h), 0);
		uint32_t ms = 0, hd = 0;
		if (g > 0 && al_inf_parse_header(h, (uint64_t)g, &ms, &hd) != 0) { ::close(fd); plain = true; return false; }
	}
	p = new AlBgzfInImpl();
	AlBgzfInImpl &I = *p;
	I.fd = fd; I.n_threads = n_threads;
	I.piece = (size_t)al_env().inflate_piece_kb << 10;      // 16 MB hold some 1 000 members of a BAM: the kernel's rate is members in flight
	I.cap_in = 2 * I.piece + 65536; I.cap_out = 4 * I.piece + 2 * 65536; I.cap_mem = I.cap_in / 64 + 1024;
	const bool host_only = al_env().test_inflate_host;
	int r = -1;
	if (!host_only) {
		r = inf_dev_open(I.dev, device, I.cap_in, I.cap_out, I.cap_mem, 2);
		if (r == 0) I.use_dev = true;
		else fprintf(stderr, "[airlift] --gpu-inflate: %s; the BGZF members are inflated by zlib on %d host thread(s) (the pieces are counted in the AL_TIMING line)\n", r > 0 ? "no device memory for the inflater's buffers" : "no usable device", n_threads);
	}
	host_backend = !I.use_dev; fell_back = !I.use_dev && !host_only;
	bool ok = true;
	for (AlBgzfInImpl::Slot &s : I.slot) {
		if (I.use_dev) {
			ok = ok && hipHostMalloc((void **)&s.h_in, I.cap_in, hipHostMallocDefault) == hipSuccess && hipHostMalloc((void **)&s.h_out, I.cap_out, hipHostMallocDefault) == hipSuccess &&
			     hipHostMalloc((void **)&s.h_mem, I.cap_mem * sizeof(AlInfMember), hipHostMallocDefault) == hipSuccess && hipHostMalloc((void **)&s.h_status, I.cap_mem * 4, hipHostMallocDefault) == hipSuccess;
		} else {
			s.h_in = (uint8_t *)malloc(I.cap_in); s.h_out = (uint8_t *)malloc(I.cap_out); s.h_mem = (AlInfMember *)malloc(I.cap_mem * sizeof(AlInfMember)); s.h_status = (uint32_t *)malloc(I.cap_mem * 4);
			ok = ok && s.h_in && s.h_out && s.h_mem && s.h_status;
		}
	}
	I.pinned = I.use_dev;
	if (!ok) { (void)hipGetLastError(); fprintf(stderr, "[ERROR] airlift: --gpu-inflate: no host memory for the reader's buffers\n"); close(); return false; }
	I.th = std::thread([this] { p->run(); });
	return true;
}

bool AlBgzfIn::read(void *dst, size_t n)
{
	AlBgzfInImpl &I = *p;
	unsigned char *d = (unsigned char *)dst;
	while (n) {
		if (I.beg == I.end) {
			const double t0 = inf_now();
			std::unique_lock<std::mutex> g(I.mu);
			if (I.have_cur) { I.slot[I.k_cons % AlBgzfInImpl::N_SLOT].state = 0; I.have_cur = false; ++I.k_cons; I.cv.notify_all(); }
			I.cv.wait(g, [&] { return I.n_made > I.k_cons || I.done; });
			I.t_wait += inf_now() - t0;
			if (I.n_made <= I.k_cons) { if (I.err) I.err_piece = std::min(I.err_piece, I.k_cons); return false; }        // the end of the file, or the piece the producer stopped at
			if (I.err && I.k_cons >= I.err_piece) return false;
			const AlBgzfInImpl::Slot &s = I.slot[I.k_cons % AlBgzfInImpl::N_SLOT];
			I.have_cur = true; I.beg = 0; I.end = s.n_out;
			continue;
		}
		const size_t t = std::min(n, I.end - I.beg);
		memcpy(d, I.slot[I.k_cons % AlBgzfInImpl::N_SLOT].h_out + I.beg, t); d += t; I.beg += t; n -= t;
	}
	return true;
}

void AlBgzfIn::timing_line(FILE *f, double scan_s) const
{
	if (!p) return;
	const AlBgzfInImpl &I = *p;
	const bool hb = !I.use_dev;
	fprintf(f, "[airlift] extract-reads: BGZF input (%s): file read %.3f s, H2D %.3f s, kernels %.3f s, D2H %.3f s, CRC %.3f s (%s), host inflate %.3f s, record scan %.3f s (+ %.3f s waiting for pieces); "
	           "%llu members in %llu pieces, %llu bytes in, %llu bytes out, %llu pieces on the host backend\n",
	        hb ? "zlib on host threads" : "k_inflate", I.t_read, I.t_h2d, I.t_kernel, I.t_d2h, I.t_crc, hb ? "zlib crc32 on the workers" : "on the device, inside the kernels' time", I.t_host,
	        scan_s - I.t_wait > 0 ? scan_s - I.t_wait : 0.0, I.t_wait, (unsigned long long)I.n_members, (unsigned long long)I.n_pieces, (unsigned long long)I.b_in, (unsigned long long)I.b_out,
	        (unsigned long long)(fell_back ? I.n_pieces : 0));
}

// ---- test taps (airlift_amd/capi.py) --------------------------------------------------------------------------------------------------------------------------
// Lists the members of src[0, n) (all of them must be whole: rc -2 when the chain breaks or the last one is cut, with what came before it still done) and
// inflates them to dst[0, *out_n), member m at the prefix sum of ISIZE, its status in status[m] (n_status words of room; rc -3 when that or cap is short).
static int inf_tap_list(const void *src, size_t n, size_t cap, size_t n_status, std::vector<AlInfMember> &mem, uint64_t *out_n, int *chain)
{
	uint64_t pos = 0; *out_n = 0;
	const int lr = al_inf_list((const uint8_t *)src, n, &pos, out_n, (uint64_t)cap, n_status, mem);
	*chain = (lr != 0 || pos != n) ? -2 : 0;
	if (lr == 0 && pos != n && mem.size() < n_status) {      // stopped at a limit, not at a cut?
		uint32_t ms = 0, hd = 0;
		if (al_inf_parse_header((const uint8_t *)src + pos, n - pos, &ms, &hd) == 0 && ms <= n - pos) return -3;
	}
	if (lr == 0 && pos != n && mem.size() >= n_status) return -3;
	return 0;
}
extern "C" int al_dbg_bgzf_inflate_host(const void *src, size_t n, void *dst, size_t cap, size_t *out_n, uint32_t *status, size_t n_status, size_t *n_members)
{
	std::vector<AlInfMember> mem; uint64_t on = 0; int chain = 0;
	if (inf_tap_list(src, n, cap, n_status, mem, &on, &chain)) return -3;
	memset(dst, 0, (size_t)on);
	for (size_t k = 0; k < mem.size(); ++k) status[k] = (uint32_t)al_inflate_member_host((const uint8_t *)src + mem[k].in_off, mem[k].msize, (uint8_t *)dst + mem[k].out_off);
	*out_n = (size_t)on; *n_members = mem.size();
	return chain;
}
static int inf_tap_dev(int device, const void *src, size_t n, void *dst, size_t cap, size_t *out_n, uint32_t *status, size_t n_status, size_t *n_members, size_t guard)
{
	std::vector<AlInfMember> mem; uint64_t on = 0; int chain = 0;
	if (inf_tap_list(src, n, cap, n_status, mem, &on, &chain)) return -3;
	*out_n = (size_t)on; *n_members = mem.size();
	if (mem.empty()) return chain;
	InfDev d;
	if (inf_dev_open(d, device, n, (size_t)on + 2 * guard + 16, mem.size(), 1) != 0) return -1;
	InfQueue &q = d.q[0];
	int rc = 0;
	std::vector<uint8_t> back((size_t)on + 2 * guard);
	if ((guard && (hipMemsetAsync(q.d_out, 0xa5, guard, q.st) != hipSuccess || hipMemsetAsync(q.d_out + guard + on, 0xa5, guard, q.st) != hipSuccess)) || (on && hipMemsetAsync(q.d_out + guard, 0, (size_t)on, q.st) != hipSuccess)) rc = -1;
	if (rc == 0 && !inf_dev_enqueue(d, 0, (const uint8_t *)src, n, mem.data(), mem.size(), back.data() + guard, (size_t)on, status, q.d_out + guard)) rc = -1;
	if (rc == 0 && !inf_dev_wait(d, 0, nullptr, nullptr, nullptr)) rc = -1;
	if (rc == 0 && guard && (hipMemcpy(back.data(), q.d_out, guard, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(back.data() + guard + on, q.d_out + guard + on, guard, hipMemcpyDeviceToHost) != hipSuccess)) rc = -1;
	inf_dev_close(d);
	if (rc) return rc;
	for (size_t i = 0; i < guard; ++i) if (back[i] != 0xa5 || back[guard + on + i] != 0xa5) return -7;      // a guard range was written
	memcpy(dst, back.data() + guard, (size_t)on);
	return chain;
}
extern "C" int al_dbg_bgzf_inflate(int device, const void *src, size_t n, void *dst, size_t cap, size_t *out_n, uint32_t *status, size_t n_status, size_t *n_members)
{
	return inf_tap_dev(device, src, n, dst, cap, out_n, status, n_status, n_members, 0);
}
// the same with the output between two poisoned guard ranges of 64 KB, checked after the kernel: -7 when one of them was written
extern "C" int al_dbg_bgzf_inflate_guard(int device, const void *src, size_t n, void *dst, size_t cap, size_t *out_n, uint32_t *status, size_t n_status, size_t *n_members)
{
	return inf_tap_dev(device, src, n, dst, cap, out_n, status, n_status, n_members, 65536);
}

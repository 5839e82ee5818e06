// al_select.hip -- --gpu-select: the reads of extract-sequence / remap selected on the GPU (the function: al_dev_select.h; the driver: al_select.h).
//
//   k_fq_select   lane per parsed record: its name hashed and probed against the name table, 0 / 1 and the bytes it will take in the arena; the
//                 selector's own grammar test lowers first_bad beside k_fq_parse's
//   (scan)        al_stream_scan_excl_u64 over the flags and over the bytes: every selected record's number and arena offset
//   k_fq_gather   wavefront per record: name, sequence (u / U -> t / T) and quality of a selected record to the arena, one descriptor each
// The text, its line index and k_fq_parse are the stream driver's (AlStreamSlot, al_stream_index_file): a backend slot IS an input-only AlStreamSlot,
// one stream each, so the copy up of one piece runs beside the kernels and the copy down of the other.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <atomic>
#include <memory>
#include "al_internal.h"
#include "al_device.h"
#include "al_runtime.h"
#include "al_stream.h"
#include "al_dev_inflate.h"
#include "al_select.h"

__global__ void __launch_bounds__(256)
k_fq_select(const uint8_t *__restrict__ t, const AlFqRec *__restrict__ rec, uint32_t n_rec, AlSelTable T, uint32_t *__restrict__ flag, uint32_t *__restrict__ bytes, unsigned long long *__restrict__ first_bad)
{
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r > n_rec) return;
	if (r == n_rec) { flag[r] = 0; bytes[r] = 0; return; }               // (the scans' last element: their totals)
	const AlFqRec q = rec[r];
	const bool sel = al_sel_probe(T, t + q.name, q.name_len);
	flag[r] = sel ? 1u : 0u; bytes[r] = sel ? al_sel_bytes(q) : 0u;
	if (al_sel_irregular(t, q)) atomicMin(first_bad, (unsigned long long)r);
}
// a wavefront per record, one byte per lane and step; a step of the second loop issues the sequence and the quality load together
__global__ void __launch_bounds__(256)
k_fq_gather(const uint8_t *__restrict__ t, const AlFqRec *__restrict__ rec, uint32_t n, const uint32_t *__restrict__ flag, const uint64_t *__restrict__ sel_off, const uint64_t *__restrict__ byte_off,
            AlSelDesc *__restrict__ desc, uint8_t *__restrict__ arena)
{
	const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
	if (r >= n || !flag[r]) return;                                      // (uniform in the wavefront)
	const AlFqRec q = rec[r];
	const uint32_t off = (uint32_t)byte_off[r];
	if (l == 0) desc[sel_off[r]] = AlSelDesc{off, q.name_len, q.len};
	uint8_t *o = arena + off;
	for (uint32_t j = l; j < q.name_len; j += 64) o[j] = t[q.name + j];
	o += q.name_len;
	for (uint32_t j = l; j < q.len; j += 64) { const uint8_t b = t[q.seq + j], c = t[q.qual + j]; o[j] = al_sel_base(b); o[q.len + j] = c; }
}

namespace {

#define SEL_CHECK(x) AL_HIP_CHECK_AS("--gpu-select", x)

struct AlSelDevBackend : AlSelBackend {
	int device = 0; bool open_ok = false, bgzf = false;
	std::atomic<size_t> own_acct{0}, *acct = &own_acct, *acct_before = nullptr;     // the account every device range of the backend is booked on
	AlStreamSlot S[2];
	AlSelSlot *d_slot = nullptr; uint8_t *d_names = nullptr; AlSelTable T{nullptr, nullptr, 0};
	DevBuf<uint32_t> flag[2], bytes[2]; DevBuf<uint64_t> sel_off[2], byte_off[2]; DevBuf<uint8_t> arena[2]; DevBuf<AlSelDesc> desc[2];
	PinnedVec<uint8_t> h_arena[2]; PinnedVec<AlSelDesc> h_desc[2];
	unsigned long long *h_cnt = nullptr;                                // page-locked: [slot * 8 ..]: first_bad, end offset, selected, bytes
	hipEvent_t ev[2][6] = {};                                          // per slot: copy up from / to, test kernels to, gather from / to, copy down to
	bool ran[2] = {false, false}, gathered[2] = {false, false};
	double up_s = 0, kernel_s = 0, down_s = 0;

	const char *name() const override { return "k_fq_select"; }
	// 0, or 1 when there is no usable device or it refuses the memory (nothing is left allocated after the destructor)
	int open(int dev, const AlSelNames &N, size_t piece)
	{
		int n_dev = 0;
		if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) { (void)hipGetLastError(); return 1; }
		device = dev < 0 ? 0 : dev;
		if (device >= n_dev || hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return 1; }
		acct_before = al_acct(); al_acct() = acct; open_ok = true;
		for (int i = 0; i < 2; ++i) {
			if (al_stream_slot_init(S[i], nullptr, device, 1)) return 1;
			for (hipEvent_t &e : ev[i]) if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); return 1; }
			if (al_stream_begin_text(S[i], 0, 2 * piece + 65536)) return 1;
		}
		if (hipHostMalloc((void **)&h_cnt, 16 * 8, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); h_cnt = nullptr; return 1; }
		if (al_dev_malloc((void **)&d_slot, N.slot.size() * sizeof(AlSelSlot)) != hipSuccess || al_dev_malloc((void **)&d_names, N.names.size()) != hipSuccess) { (void)hipGetLastError(); return 1; }
		if (hipMemcpy(d_slot, N.slot.data(), N.slot.size() * sizeof(AlSelSlot), hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_names, N.names.data(), N.names.size(), hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); return 1; }
		T = AlSelTable{d_slot, d_names, (uint32_t)N.slot.size() - 1};
		return 0;
	}
	int bgzf_init(size_t cap_in, size_t cap_mem) { bgzf = true; for (int i = 0; i < 2; ++i) if (al_stream_bgzf_init(S[i], cap_in, cap_mem)) return 1; return 0; }
	~AlSelDevBackend() override
	{
		if (!open_ok) return;
		(void)hipSetDevice(device);
		for (int i = 0; i < 2; ++i) {
			if (S[i].io) (void)hipStreamSynchronize(S[i].io);
			flag[i].release(); bytes[i].release(); sel_off[i].release(); byte_off[i].release(); arena[i].release(); desc[i].release();
			al_stream_slot_destroy(S[i]);
			for (hipEvent_t &e : ev[i]) if (e) (void)hipEventDestroy(e);
		}
		if (d_slot) al_dev_free(d_slot); if (d_names) al_dev_free(d_names);
		if (h_cnt) (void)hipHostFree(h_cnt);
		al_acct() = acct_before;
	}
	size_t held() const override { return acct->load(); }

	int begin(int s, size_t cap) override
	{
		if (al_stream_begin_text(S[s], 0, cap)) return -1;
		ran[s] = gathered[s] = false;
		SEL_CHECK(hipEventRecord(ev[s][0], S[s].io));
		return 0;
	}
	int room(int s, uint64_t n) const { if (S[s].txt_n[0] + n + 4096 + 16 > S[s].txt[0].cap) { fprintf(stderr, "[airlift] --gpu-select: text buffer too small\n"); return -1; } return 0; }
	int carry(int s, int from, uint64_t off, uint64_t n) override
	{
		if (n == 0) return 0;
		if (room(s, n)) return -1;
		SEL_CHECK(hipMemcpyAsync(S[s].txt[0].p + S[s].txt_n[0], S[from].txt[0].p + off, n, hipMemcpyDeviceToDevice, S[s].io));
		S[s].txt_n[0] += n;
		return 0;
	}
	int append(int s, const uint8_t *p, size_t n) override
	{
		if (n == 0) return 0;
		if (room(s, n)) return -1;
		SEL_CHECK(hipMemcpyAsync(S[s].txt[0].p + S[s].txt_n[0], p, n, hipMemcpyHostToDevice, S[s].io));
		S[s].txt_n[0] += n;
		return 0;
	}
	int append_bgzf(int s, const uint8_t *b, size_t n_in, const AlInfMember *mem, size_t n_mem, uint64_t n_out, size_t *bad, uint32_t *bad_status) override
	{
		return al_stream_append_bgzf(S[s], 0, b, n_in, mem, n_mem, n_out, bad, bad_status);
	}
	int end_text(int s) override { return al_stream_end_text(S[s], 0); }
	uint64_t text_bytes(int s) const override { return S[s].txt_n[0]; }
	int select(int s, AlSelPiece *r) override
	{
		AlStreamSlot &X = S[s]; hipStream_t st = X.io;
		SEL_CHECK(hipSetDevice(device));
		SEL_CHECK(hipEventRecord(ev[s][1], st));
		uint64_t lines = 0;
		if (al_stream_index_file(X, 0, &lines)) return -1;
		*r = AlSelPiece(); r->lines = lines; r->n_rec = lines / 4;
		const uint32_t n = (uint32_t)r->n_rec;
		if (flag[s].ensure((size_t)n + 2) || bytes[s].ensure((size_t)n + 2) || sel_off[s].ensure((size_t)n + 2) || byte_off[s].ensure((size_t)n + 2)) return -1;
		hipLaunchKernelGGL(k_fq_select, dim3((n + 256) / 256), dim3(256), 0, st, X.txt[0].p, X.frec[0].p, n, T, flag[s].p, bytes[s].p, X.st.p + 2);
		if (al_stream_scan_excl_u64(X, flag[s].p, sel_off[s].p, (size_t)n + 1, st) || al_stream_scan_excl_u64(X, bytes[s].p, byte_off[s].p, (size_t)n + 1, st)) return -1;
		SEL_CHECK(hipEventRecord(ev[s][2], st));
		unsigned long long *h = h_cnt + 8 * s; uint32_t *h_end = (uint32_t *)(h + 1);
		auto fetch = [&](uint64_t k) -> int {
			SEL_CHECK(hipMemcpyAsync(h_end, X.ls[0].p + 4 * k, 4, hipMemcpyDeviceToHost, st));
			SEL_CHECK(hipMemcpyAsync(h + 2, sel_off[s].p + k, 8, hipMemcpyDeviceToHost, st));
			SEL_CHECK(hipMemcpyAsync(h + 3, byte_off[s].p + k, 8, hipMemcpyDeviceToHost, st));
			SEL_CHECK(hipStreamSynchronize(st));
			return 0;
		};
		SEL_CHECK(hipMemcpyAsync(h, X.st.p + 2, 8, hipMemcpyDeviceToHost, st));
		if (fetch(r->n_rec)) return -1;
		r->first_bad = h[0];
		r->n_take = r->n_rec < r->first_bad ? r->n_rec : r->first_bad;
		if (r->n_take != r->n_rec && fetch(r->n_take)) return -1;        // (irregular input: the counts in front of the first bad record)
		r->consumed = *h_end; r->n_sel = h[2]; r->arena_bytes = h[3];
		SEL_CHECK(hipGetLastError());
		ran[s] = true;
		return 0;
	}
	int gather(int s, const AlSelPiece &r) override
	{
		AlStreamSlot &X = S[s]; hipStream_t st = X.io;
		if (arena[s].ensure((size_t)r.arena_bytes + 16) || desc[s].ensure((size_t)r.n_sel + 1) || h_arena[s].resize((size_t)r.arena_bytes + 1) || h_desc[s].resize((size_t)r.n_sel + 1)) return -1;
		SEL_CHECK(hipEventRecord(ev[s][3], st));
		if (r.n_take && r.n_sel) hipLaunchKernelGGL(k_fq_gather, dim3((unsigned)((r.n_take + 3) / 4)), dim3(256), 0, st, X.txt[0].p, X.frec[0].p, (uint32_t)r.n_take, flag[s].p, sel_off[s].p, byte_off[s].p, desc[s].p, arena[s].p);
		SEL_CHECK(hipEventRecord(ev[s][4], st));
		if (r.arena_bytes) SEL_CHECK(hipMemcpyAsync(h_arena[s].data(), arena[s].p, (size_t)r.arena_bytes, hipMemcpyDeviceToHost, st));
		if (r.n_sel) SEL_CHECK(hipMemcpyAsync(h_desc[s].data(), desc[s].p, (size_t)r.n_sel * sizeof(AlSelDesc), hipMemcpyDeviceToHost, st));
		SEL_CHECK(hipEventRecord(ev[s][5], st));
		SEL_CHECK(hipGetLastError());
		gathered[s] = true;
		return 0;
	}
	int finish(int s, const uint8_t **a, const AlSelDesc **d) override
	{
		SEL_CHECK(hipStreamSynchronize(S[s].io));
		*a = h_arena[s].data(); *d = h_desc[s].data();
		if (ran[s] && gathered[s]) {
			float ms[4] = {0, 0, 0, 0};
			if (hipEventElapsedTime(&ms[0], ev[s][0], ev[s][1]) == hipSuccess && hipEventElapsedTime(&ms[1], ev[s][1], ev[s][2]) == hipSuccess &&
			    hipEventElapsedTime(&ms[2], ev[s][3], ev[s][4]) == hipSuccess && hipEventElapsedTime(&ms[3], ev[s][4], ev[s][5]) == hipSuccess) { up_s += ms[0] * 1e-3; kernel_s += (ms[1] + ms[2]) * 1e-3; down_s += ms[3] * 1e-3; }
			else (void)hipGetLastError();
		}
		return 0;
	}
	void *host_buffer(size_t n) override { void *p = nullptr; if (hipHostMalloc(&p, n, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; } return p; }
	void host_buffer_free(void *p) override { (void)hipHostFree(p); }
	int fetch_flags(int s, uint32_t *dst, size_t n) override { if (n) SEL_CHECK(hipMemcpy(dst, flag[s].p, n * 4, hipMemcpyDeviceToHost)); return 0; }
	void stat(AlSelStat &st) override { st.up_s += up_s; st.kernel_s += kernel_s; st.down_s += down_s; }
};

// BGZF (its first bytes pass al_inf_parse_header): 1; another gzip file, or "-": 2; anything else: 0
int sel_file_kind(const char *fn)
{
	if (!strcmp(fn, "-")) return 2;
	const int fd = open(fn, O_RDONLY);
	if (fd < 0) return 0;
	uint8_t h[4096]; int k = 0;
	const ssize_t g = pread(fd, h, sizeof(h), 0);
	uint32_t ms = 0, hd = 0;
	if (g >= 2 && h[0] == 0x1f && h[1] == 0x8b) k = al_inf_parse_header(h, (uint64_t)g, &ms, &hd) == 0 ? 1 : 2;
	close(fd);
	return k;
}

} // namespace

int al_select_subseq(const char *fn, const AlSelNames &N, bool host_backend, bool gpu_inflate, int device, size_t piece_bytes, const AlSelEmit &emit,
                     uint64_t *handover, AlSelStat *st, const char **backend, size_t *held)
{
	*handover = ~0ull; *held = 0;
	const int kind = sel_file_kind(fn);
	const size_t zpiece = (size_t)al_env().inflate_piece_kb << 10, zcap = 2 * zpiece + 65536, zmem = zcap / 64 + 1024;
	// the default piece: 8 MB of a plain file; of a BGZF file four compressed pieces' worth of text, since k_inflate's rate is members in flight
	if (piece_bytes == 0) piece_bytes = kind == 1 ? std::max((size_t)8 << 20, 4 * zpiece) : (size_t)8 << 20;
	if (piece_bytes >= ((size_t)1 << 29)) piece_bytes = (size_t)1 << 29;
	if (kind == 2 || (kind == 1 && !gpu_inflate)) {
		fprintf(stderr, "[airlift] --gpu-select: '%s' is %s; it is read as one gzip stream on the host\n", fn, kind == 2 ? "not a BGZF file" : "a BGZF file and --gpu-inflate is not given");
		return 1;
	}
	const int fd = open(fn, O_RDONLY);
	if (fd < 0) { fprintf(stderr, "ERROR: failed to open file '%s'\n", fn); return -1; }
	int rc = -1;
	std::atomic<size_t> acct{0};
	{
		std::unique_ptr<AlSelBackend> B;
		if (!host_backend) {
			std::unique_ptr<AlSelDevBackend> D(new AlSelDevBackend()); D->acct = &acct;
			int r = D->open(device, N, piece_bytes);
			if (r == 0 && kind == 1) r = D->bgzf_init(zcap, zmem);
			if (r == 0) B = std::move(D);
			else { static std::atomic<bool> said{false}; if (!said.exchange(true)) fprintf(stderr, "[airlift] --gpu-select: no usable device, or no device memory for the selector's buffers; the host twin selects the reads\n"); }
		}
		if (!B) B.reset(new AlSelHostBackend(N.table()));
		*backend = B->name();
		if (kind == 1) {
			AlSelBgzfSource src; src.fd = fd; src.B = B.get(); src.fn = fn;
			if (src.open(zpiece) == 0) { src.max_in = zcap; src.max_mem = zmem; rc = al_select_file(*B, src, piece_bytes, emit, handover, *st); }
		} else {
			AlSelPlainSource src; src.fd = fd; src.B = B.get(); src.fn = fn;
			rc = al_select_file(*B, src, piece_bytes, emit, handover, *st);
		}
		B->stat(*st);
		B.reset();                                                      // every device range goes back here
	}
	close(fd);
	*held = acct.load();
	return rc;
}

// ---- test taps (airlift_amd/capi.py) ------------------------------------------------------------------------------------------------------------------------------
// One text and one list of names (each followed by '\n') through ONE pass of a backend: flags[0, *n_rec) (n_flags of room), *first_bad (~0: none), the arena
// and the descriptors (three words each: offset, name length, sequence length) of the selected records in front of first_bad.  0; -1 a device failure; -3 room.
static int sel_tap(AlSelBackend &B, const void *text, size_t n, uint32_t *flags, size_t n_flags, uint64_t *n_rec, uint64_t *first_bad,
                   void *arena, size_t arena_cap, size_t *arena_n, uint32_t *desc, size_t desc_cap, size_t *n_sel)
{
	AlSelPiece r; const uint8_t *a = nullptr; const AlSelDesc *d = nullptr;
	if (B.begin(0, n + 1) || B.append(0, (const uint8_t *)text, n) || B.end_text(0) || B.select(0, &r)) return -1;
	*n_rec = r.n_rec; *first_bad = r.first_bad; *arena_n = (size_t)r.arena_bytes; *n_sel = (size_t)r.n_sel;
	if (r.n_rec > n_flags || r.arena_bytes > arena_cap || r.n_sel > desc_cap) return -3;
	if (B.gather(0, r) || B.finish(0, &a, &d) || B.fetch_flags(0, flags, (size_t)r.n_rec)) return -1;
	if (r.arena_bytes) memcpy(arena, a, (size_t)r.arena_bytes);
	for (size_t k = 0; k < (size_t)r.n_sel; ++k) { desc[3 * k] = d[k].off; desc[3 * k + 1] = d[k].name_len; desc[3 * k + 2] = d[k].len; }
	return 0;
}
static int sel_tap_names(const char *names, size_t names_len, AlSelNames &N)
{
	std::vector<std::string> v; std::vector<std::string> uniq;
	for (size_t p = 0; p < names_len; ) { const char *q = (const char *)memchr(names + p, '\n', names_len - p); const size_t e = q ? (size_t)(q - names) : names_len; v.emplace_back(names + p, e - p); p = e + 1; }
	std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end());
	return al_sel_build(v, N);
}
extern "C" int al_dbg_fq_select_host(const void *text, size_t n, const char *names, size_t names_len, uint32_t *flags, size_t n_flags, uint64_t *n_rec, uint64_t *first_bad,
                                     void *arena, size_t arena_cap, size_t *arena_n, uint32_t *desc, size_t desc_cap, size_t *n_sel)
{
	AlSelNames N;
	if (sel_tap_names(names, names_len, N)) return -3;
	AlSelHostBackend B(N.table());
	return sel_tap(B, text, n, flags, n_flags, n_rec, first_bad, arena, arena_cap, arena_n, desc, desc_cap, n_sel);
}
extern "C" int al_dbg_fq_select(int device, const void *text, size_t n, const char *names, size_t names_len, uint32_t *flags, size_t n_flags, uint64_t *n_rec, uint64_t *first_bad,
                                void *arena, size_t arena_cap, size_t *arena_n, uint32_t *desc, size_t desc_cap, size_t *n_sel)
{
	AlSelNames N;
	if (sel_tap_names(names, names_len, N)) return -3;
	if (n >= ((size_t)1 << 31) - 65536) return -3;
	AlSelDevBackend B;
	if (B.open(device, N, n / 2 + 1)) return -1;
	return sel_tap(B, text, n, flags, n_flags, n_rec, first_bad, arena, arena_cap, arena_n, desc, desc_cap, n_sel);
}

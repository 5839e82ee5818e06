// al_bai.hip -- `bam-index`: the BAI of a coordinate-sorted BAM built on the GPU (the function: al_dev_bai.h; the driver and the file's assembly: al_bai.h).
//
// Per piece, on the backend's stream:
//   k_inflate      al_stream_append_bgzf, as `lift` and `merge` launch it: the piece's members inflated to the text's end
//   k_bam_walk     al_dev_walk.h, as it is: the record offsets of the text
//   k_bai_key      lane per record: al_bai_record -- the fixed fields read byte-wise (records are not aligned), the CIGAR words walked for reflen, the interval, the
//                  2^29 and LN checks, reg2bin, and two binary searches of the piece's member table for the virtual offsets of the record's start and end; the first
//                  refused record (number << 8 | code) by atomicMin.  The descent check is made here too: nothing is patched, so a lane reads the key fields of the
//                  record before its own (record 0: the last key of the piece before, passed in); descents counted with one atomic per wavefront, the smallest
//                  offset of one by atomicMin
//   k_bai_heads    lane per record: 1 where (refID, bin) differs from the record before -- a run starts; al_stream_scan_excl_u64 over the flags numbers the runs
//   k_bai_rows     lane per record: a run's head writes (refID, bin, start offset) of its row, a run's last record the row's end offset
//   k_bai_lin      lane per record: the per-contig counts -- the input is in order, so a wavefront holds few contigs: per contig it touches, one ballot and one
//                  atomic per count by the contig's first lane -- and the linear index: for each window a record with flag 4 clear touches, a plain load and a
//                  64-bit atomicMin only when the lane's offset is smaller; the result does not depend on the order of the lanes
// The rows come down with each piece (the driver joins the open run across pieces); the linear index and the counts stay on the device until the last piece.  Every
// store is a vector store.  The kernels are small beside inflate and walk, which bound the pass on lift's evidence; nothing here is MEASURED yet.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <atomic>
#include <memory>
#include <string>
#include "al_internal.h"
#include "al_device.h"
#include "al_runtime.h"
#include "al_stream.h"
#include "al_dev_inflate.h"
#include "al_bai.h"
#include "al_dev_walk.h"
#include "al_env.h"
#include "../../include/airlift.h"

// st[0]: the first refused record << 8 | its code, st[1]: descents, st[2]: the smallest offset of a record below its predecessor, st[3]: the last record's key
__global__ void __launch_bounds__(256)
k_bai_key(const uint8_t *__restrict__ t, const uint32_t *__restrict__ rec_off, uint32_t n_rec, uint64_t base, uint32_t n_ref, const uint32_t *__restrict__ ref_len,
          const AlBaiMember *__restrict__ mem, uint32_t n_mem, uint32_t has_prev, uint64_t prev_key, AlBaiRec *__restrict__ rec, unsigned long long *__restrict__ st)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	bool d = false;
	if (i < n_rec) {
		AlBaiRec o; uint64_t key;
		const uint32_t off = rec_off[i], code = al_bai_record(t, off, base, n_ref, ref_len, mem, n_mem, &o, &key);
		rec[i] = o;
		if (code) atomicMin(st, (unsigned long long)i << 8 | code);
		uint32_t c0;
		const uint64_t before = i ? al_bai_key(t + rec_off[i - 1], n_ref, &c0) : prev_key;
		d = (i || has_prev) && key < before;
		if (d) atomicMin(st + 2, (unsigned long long)off);
		if (i == n_rec - 1) st[3] = key;
	}
	const unsigned long long m = __ballot(d);
	if ((threadIdx.x & 63) == 0 && m) atomicAdd(st + 1, (unsigned long long)__popcll(m));
}
__global__ void __launch_bounds__(256)
k_bai_heads(const AlBaiRec *__restrict__ rec, uint32_t n_rec, uint32_t *__restrict__ head)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n_rec) head[i] = al_bai_head(rec, i) ? 1u : 0u;
	else if (i == n_rec) head[i] = 0;                                   // (the scan's last element: the total)
}
__global__ void __launch_bounds__(256)
k_bai_rows(const AlBaiRec *__restrict__ rec, uint32_t n_rec, const uint32_t *__restrict__ head, const uint64_t *__restrict__ before, AlBaiRow *__restrict__ rows)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_rec) return;
	const uint32_t h = head[i]; const uint64_t run = before[i] + h - 1;       // (record 0 is a head: run >= 0)
	const AlBaiRec x = rec[i];
	if (h) { rows[run].ref = x.ref; rows[run].bin = x.bin; rows[run].beg = x.vbeg; }
	if (i + 1 == n_rec || head[i + 1]) rows[run].end = x.vend;
}
__global__ void __launch_bounds__(256)
k_bai_lin(const AlBaiRec *__restrict__ rec, uint32_t n_rec, uint32_t n_ref, const uint64_t *__restrict__ lin_off, unsigned long long *__restrict__ lin, unsigned long long *__restrict__ cnt)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
	const bool valid = i < n_rec;
	int32_t ref = -1; uint32_t win = 0; uint64_t vbeg = 0;
	if (valid) { const AlBaiRec x = rec[i]; ref = x.ref; win = x.win; vbeg = x.vbeg; }
	const bool mapped = win >> 31;
	unsigned long long todo = __ballot(valid);
	while (todo) {                                                      // (uniform: one turn per contig the wavefront holds)
		const int leader = __ffsll((long long)todo) - 1;
		const int32_t r = __shfl(ref, leader);
		const unsigned long long same = __ballot(valid && ref == r), mm = __ballot(valid && ref == r && mapped);
		if ((int)lane == leader) {
			if (r < 0) atomicAdd(cnt + 2 * (size_t)n_ref, (unsigned long long)__popcll(same));
			else {
				if (mm) atomicAdd(cnt + 2 * (size_t)r, (unsigned long long)__popcll(mm));
				if (same & ~mm) atomicAdd(cnt + 2 * (size_t)r + 1, (unsigned long long)__popcll(same & ~mm));
			}
		}
		todo &= ~same;
	}
	if (valid && ref >= 0 && mapped) {
		unsigned long long *p = lin + lin_off[ref];                      // (al_bai_record: the last window lies below the contig's al_bai_n_win)
		for (uint32_t w = win & 0x7fff, w1 = (win >> 16) & 0x7fff; w <= w1; ++w) if (vbeg < p[w]) atomicMin(p + w, (unsigned long long)vbeg);
	}
}

namespace {

#define BAI_CHECK(x) AL_HIP_CHECK_AS("bam-index", x)
static inline double bai_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct AlBaiDevBackend : AlBaiBackend {
	int device = 0; bool open_ok = false;
	std::atomic<size_t> own_acct{0}, *acct = &own_acct, *acct_before = nullptr;      // the account every device range of the backend is booked on
	AlStreamSlot S; int at = 0;
	DevBuf<uint32_t> rec_off, head, d_len; DevBuf<uint64_t> before, d_lin_off; DevBuf<unsigned long long> d_lin, d_cnt, st;   // st: the four status words, the walk's three words behind them
	DevBuf<AlBaiRec> rec; DevBuf<AlBaiRow> d_rows; DevBuf<AlBaiMember> d_mem;
	unsigned long long *h_st = nullptr;                                 // page-locked: 8 words
	AlBaiTables T;                                                      // ref_len and lin_off; lin and cnt are filled by tables()
	double up_s = 0, walk_s = 0, key_s = 0;

	const char *name() const override { return "k_bai"; }
	// 0, or 1 when there is no usable device or it refuses the memory (nothing is left allocated after the destructor)
	int open(int dev, size_t cap_in, size_t cap_mem)
	{
		int n_dev = 0;
		if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) { (void)hipGetLastError(); return 1; }
		device = dev < 0 ? 0 : dev;
		if (device >= n_dev || hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return 1; }
		acct_before = al_acct(); al_acct() = acct; open_ok = true;
		if (al_stream_slot_init(S, nullptr, device, 2)) return 1;
		if (st.ensure(8)) return 1;
		if (cap_in && al_stream_bgzf_init(S, cap_in, cap_mem)) return 1;
		if (hipHostMalloc((void **)&h_st, 8 * 8, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); h_st = nullptr; return 1; }
		return 0;
	}
	~AlBaiDevBackend() override
	{
		if (!open_ok) return;
		(void)hipSetDevice(device);
		if (S.io) (void)hipStreamSynchronize(S.io);
		rec_off.release(); head.release(); d_len.release(); before.release(); d_lin_off.release(); d_lin.release(); d_cnt.release(); st.release(); rec.release(); d_rows.release(); d_mem.release();
		al_stream_slot_destroy(S);
		if (h_st) (void)hipHostFree(h_st);
		al_acct() = acct_before;
	}
	size_t held() const override { return acct->load(); }

	int set_refs(const uint32_t *len, uint32_t n_ref) override
	{
		BAI_CHECK(hipSetDevice(device));
		T.set(len, n_ref);
		const size_t n_lin = T.lin.size();
		if (d_len.ensure((size_t)n_ref + 1) || d_lin_off.ensure((size_t)n_ref + 1) || d_lin.ensure(n_lin + 1) || d_cnt.ensure(2 * (size_t)n_ref + 1)) return -1;
		if (n_ref) BAI_CHECK(hipMemcpyAsync(d_len.p, len, (size_t)n_ref * 4, hipMemcpyHostToDevice, S.io));
		BAI_CHECK(hipMemcpyAsync(d_lin_off.p, T.lin_off.data(), ((size_t)n_ref + 1) * 8, hipMemcpyHostToDevice, S.io));
		BAI_CHECK(hipMemsetAsync(d_lin.p, 0xff, (n_lin + 1) * 8, S.io));
		BAI_CHECK(hipMemsetAsync(d_cnt.p, 0, (2 * (size_t)n_ref + 1) * 8, S.io));
		BAI_CHECK(hipStreamSynchronize(S.io));
		return 0;
	}
	int begin(size_t cap) override
	{
		BAI_CHECK(hipSetDevice(device));
		at ^= 1;
		return al_stream_begin_text(S, at, cap + 2 * AL_LIFT_W) ? -1 : 0;       // (room for k_bam_walk to load whole windows)
	}
	int room(uint64_t n) const { if (S.txt_n[at] + n + 16 > S.txt[at].cap) { fprintf(stderr, "[airlift] bam-index: text buffer too small\n"); return -1; } return 0; }
	int carry(uint64_t off, uint64_t n) override
	{
		if (n == 0) return 0;
		const int a = at, o = a ^ 1;
		if (room(n) || off + n > S.txt_n[o]) return -1;
		BAI_CHECK(hipMemcpyAsync(S.txt[a].p + S.txt_n[a], S.txt[o].p + off, n, hipMemcpyDeviceToDevice, S.io));
		S.txt_n[a] += n;
		return 0;
	}
	int append(const uint8_t *p, size_t n) override
	{
		if (n == 0) return 0;
		if (room(n)) return -1;
		BAI_CHECK(hipMemcpyAsync(S.txt[at].p + S.txt_n[at], p, n, hipMemcpyHostToDevice, S.io));
		BAI_CHECK(hipStreamSynchronize(S.io));
		S.txt_n[at] += n;
		return 0;
	}
	int append_bgzf(const uint8_t *b, size_t n_in, const AlInfMember *mem, size_t n_mem, uint64_t n_out, size_t *bad, uint32_t *bad_status) override
	{
		const double t0 = bai_now(), k0 = S.bz.kernel_s;
		const int r = al_stream_append_bgzf(S, at, b, n_in, mem, n_mem, n_out, bad, bad_status);
		up_s += bai_now() - t0 - (S.bz.kernel_s - k0);
		return r;
	}
	uint64_t text_bytes() const override { return S.txt_n[at]; }
	int run(uint64_t start, uint64_t base, const AlBaiMember *mem, size_t n_mem, bool has_prev, uint64_t prev_key, AlBaiPiece *r, std::vector<AlBaiRow> &rows) override
	{
		hipStream_t q = S.io; const int a = at;
		BAI_CHECK(hipSetDevice(device));
		*r = AlBaiPiece(); rows.clear();
		const uint64_t n = S.txt_n[a];
		if (n >= (1ull << 31) || start > n || n_mem >= (1ull << 31)) { fprintf(stderr, "[airlift] bam-index: a text of %llu bytes\n", (unsigned long long)n); return -1; }
		const double t0 = bai_now();
		if (rec_off.ensure((size_t)(n / 36) + 64) || d_mem.ensure(n_mem + 1)) return -1;      // (a record takes at least 36 bytes)
		uint32_t *hw = (uint32_t *)(h_st + 4);
		h_st[0] = ~0ull; h_st[1] = 0; h_st[2] = ~0ull; h_st[3] = 0;
		BAI_CHECK(hipMemcpyAsync(st.p, h_st, 32, hipMemcpyHostToDevice, q));
		if (n_mem) BAI_CHECK(hipMemcpyAsync(d_mem.p, mem, n_mem * sizeof(AlBaiMember), hipMemcpyHostToDevice, q));
		hipLaunchKernelGGL(k_bam_walk, dim3(1), dim3(64), 0, q, S.txt[a].p, (uint32_t)n, (uint32_t)std::min<size_t>(S.txt[a].cap, 0xfffffff0u), (uint32_t)start, rec_off.p, (uint32_t *)(st.p + 4));
		BAI_CHECK(hipMemcpyAsync(hw, st.p + 4, 12, hipMemcpyDeviceToHost, q));
		BAI_CHECK(hipStreamSynchronize(q));
		BAI_CHECK(hipGetLastError());
		const double t1 = bai_now(); walk_s += t1 - t0;
		const uint32_t nr = hw[0];
		r->n_rec = nr; r->consumed = hw[1]; r->walk_bad = hw[2];
		if (nr == 0) return 0;
		if (rec.ensure((size_t)nr + 1) || head.ensure((size_t)nr + 2) || before.ensure((size_t)nr + 2) || d_rows.ensure((size_t)nr + 1)) return -1;
		const dim3 g((nr + 255) / 256), g1((nr + 256) / 256), b(256);
		hipLaunchKernelGGL(k_bai_key, g, b, 0, q, S.txt[a].p, rec_off.p, nr, base, (uint32_t)T.ref_len.size(), d_len.p, d_mem.p, (uint32_t)n_mem, has_prev ? 1u : 0u, prev_key, rec.p, st.p);
		BAI_CHECK(hipMemcpyAsync(h_st, st.p, 32, hipMemcpyDeviceToHost, q));
		BAI_CHECK(hipStreamSynchronize(q));
		BAI_CHECK(hipGetLastError());
		r->descents = h_st[1]; r->desc_off = h_st[2]; r->last_key = h_st[3];
		if (h_st[0] != ~0ull) {
			r->first_bad = h_st[0] >> 8; r->bad_code = (uint32_t)(h_st[0] & 0xff);
			uint32_t off = 0; BAI_CHECK(hipMemcpy(&off, rec_off.p + r->first_bad, 4, hipMemcpyDeviceToHost)); r->bad_off = off;
		}
		if (r->first_bad != ~0ull || r->descents) { key_s += bai_now() - t1; return 0; }      // (the driver refuses the piece: no rows, and the tables are not touched)
		hipLaunchKernelGGL(k_bai_heads, g1, b, 0, q, rec.p, nr, head.p);
		hipLaunchKernelGGL(k_bai_lin, g, b, 0, q, rec.p, nr, (uint32_t)T.ref_len.size(), d_lin_off.p, d_lin.p, d_cnt.p);
		if (al_stream_scan_excl_u64(S, head.p, before.p, (size_t)nr + 1, q)) return -1;
		hipLaunchKernelGGL(k_bai_rows, g, b, 0, q, rec.p, nr, head.p, before.p, d_rows.p);
		BAI_CHECK(hipMemcpyAsync(h_st + 6, before.p + nr, 8, hipMemcpyDeviceToHost, q));
		BAI_CHECK(hipStreamSynchronize(q));
		BAI_CHECK(hipGetLastError());
		const uint64_t n_rows = h_st[6];
		if (n_rows == 0 || n_rows > nr) { fprintf(stderr, "[airlift] bam-index: %llu runs of %u records\n", (unsigned long long)n_rows, nr); return -1; }
		rows.resize((size_t)n_rows);
		BAI_CHECK(hipMemcpy(rows.data(), d_rows.p, (size_t)n_rows * sizeof(AlBaiRow), hipMemcpyDeviceToHost));
		key_s += bai_now() - t1;
		return 0;
	}
	int tables(AlBaiTables &o) override
	{
		BAI_CHECK(hipSetDevice(device));
		o = T;
		if (!o.lin.empty()) BAI_CHECK(hipMemcpy(o.lin.data(), d_lin.p, o.lin.size() * 8, hipMemcpyDeviceToHost));
		BAI_CHECK(hipMemcpy(o.cnt.data(), d_cnt.p, o.cnt.size() * 8, hipMemcpyDeviceToHost));
		return 0;
	}
	void *host_buffer(size_t n) override { void *p = nullptr; if (hipHostMalloc(&p, n, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; } return p; }
	void host_buffer_free(void *p) override { (void)hipHostFree(p); }
	void stat(AlBaiRun &s) override { s.up_s += up_s; s.walk_s += walk_s; s.key_s += key_s; s.inflate_s += S.bz.kernel_s; }
};

// One attempt with one backend.  0; -1; -2 refused input; *nomem: the device refused memory (the caller runs the twin)
int bai_once(int fd, const char *bam, const AlLiftHeader &H, uint64_t file_off, uint64_t out_off, uint64_t start, bool host_backend, int device, int n_threads, size_t piece_bytes,
             AlBaiRun &run, const char **backend, std::atomic<size_t> &acct, std::vector<uint8_t> &bai, bool *nomem)
{
	*nomem = false;
	const size_t zpiece = (size_t)al_env().inflate_piece_kb << 10, zcap = 2 * zpiece + 65536, zmem = zcap / 64 + 1024;
	if (piece_bytes == 0) piece_bytes = std::max((size_t)8 << 20, 4 * zpiece);
	if (piece_bytes >= ((size_t)1 << 29)) piece_bytes = (size_t)1 << 29;
	std::unique_ptr<AlBaiBackend> B; AlBaiDevBackend *D = nullptr;
	if (!host_backend) {
		std::unique_ptr<AlBaiDevBackend> d(new AlBaiDevBackend()); d->acct = &acct;
		if (d->open(device, zcap, zmem) == 0) { D = d.get(); B = std::move(d); }
		else { al_nomem_flag() = false; fprintf(stderr, "[airlift] bam-index: no usable device, or no device memory for the index's buffers; the host twin builds the index\n"); }
	}
	if (!B) B.reset(new AlBaiHostBackend(n_threads));
	*backend = D ? "k_bai" : "host twin";
	int rc = -1;
	{
		AlBaiAcc A; AlBaiPort port; port.B = B.get(); port.A = &A; port.s_at = out_off; port.f_at = file_off;
		AlBaiBgzfSource src; src.fd = fd; src.B = &port; src.fn = bam;
		if (B->set_refs(H.len.data(), (uint32_t)H.len.size()) == 0 && src.open(zpiece, file_off, out_off) == 0) {
			src.max_in = zcap; src.max_mem = zmem;
			rc = al_bai_stream(*B, src, port, piece_bytes, start, out_off, bam, A, run);
			if (rc == 0) {
				const double t0 = bai_now();
				AlBaiTables T;
				if (B->tables(T)) rc = -1;
				else { al_bai_assemble(A.rows, T, bai, &run.chunks); run.unplaced = T.cnt.back(); }
				run.assemble_s += bai_now() - t0;
			}
		}
	}                                                                   // (the source's page-locked window goes back through the backend)
	B->stat(run);
	B.reset();                                                          // every device range goes back here
	if (rc == -1 && D && al_nomem_flag()) { al_nomem_flag() = false; *nomem = true; }
	return rc;
}

} // namespace

int al_bai_index_file(const char *bam, const char *bai_fn, bool host_backend, int device, int n_threads, size_t piece_bytes, AlBaiRun *run_out, size_t *held, bool *on_device)
{
	const auto t_wall = std::chrono::steady_clock::now();
	const std::string out = bai_fn ? std::string(bai_fn) : std::string(bam) + ".bai", tmp = out + ".tmp." + std::to_string((long)getpid());
	if (out == bam) { fprintf(stderr, "[ERROR] airlift: bam-index: the input '%s' is also the output\n", bam); return -1; }
	const int fd = open(bam, O_RDONLY);
	if (fd < 0) { fprintf(stderr, "ERROR: failed to open file '%s'\n", bam); return -1; }
	AlLiftHeader H; uint64_t file_off = 0, out_off = 0, start = 0;
	int rc = lift_read_header(fd, bam, H, &file_off, &out_off, &start, "bam-index");
	if (rc) { close(fd); return rc; }
	std::atomic<size_t> acct{0}; AlBaiRun run; const char *backend = ""; bool nomem = false; std::vector<uint8_t> bai;
	rc = bai_once(fd, bam, H, file_off, out_off, start, host_backend, device, n_threads, piece_bytes, run, &backend, acct, bai, &nomem);
	if (rc && nomem) {
		fprintf(stderr, "[airlift] bam-index: the device refused memory during the pass; the host twin builds the index from the start\n");
		run = AlBaiRun();
		rc = bai_once(fd, bam, H, file_off, out_off, start, true, device, n_threads, piece_bytes, run, &backend, acct, bai, &nomem);
	}
	close(fd);
	if (rc == 0) {                                                      // a temporary name beside the target, then the rename: no partial index is ever seen
		const double t0 = bai_now();
		FILE *fo = fopen(tmp.c_str(), "wb");
		const bool ok = fo && fwrite(bai.data(), 1, bai.size(), fo) == bai.size();
		if ((fo && fclose(fo) == EOF) || !ok || rename(tmp.c_str(), out.c_str()) != 0) { fprintf(stderr, "[ERROR] failed to write the output to file '%s'\n", out.c_str()); if (fo) unlink(tmp.c_str()); rc = -1; }
		run.bai_bytes = bai.size(); run.assemble_s += bai_now() - t0;
	}
	const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_wall).count();
	if (run_out) *run_out = run;
	if (held) *held = acct.load();
	if (on_device) *on_device = strcmp(backend, "host twin") != 0;
	if (rc == 0 && al_env().timing)
		fprintf(stderr, "[airlift] bam-index: '%s' into '%s' (%s): %llu records, %llu without a contig, %llu pieces, %llu bytes in, %llu chunks, %llu bytes of index; file read %.3f s, copy up %.3f s, inflate %.3f s, walk %.3f s, keys %.3f s, assemble %.3f s, wall %.3f s; device bytes held at return: %zu\n",
		        bam, out.c_str(), backend, (unsigned long long)run.records, (unsigned long long)run.unplaced, (unsigned long long)run.pieces, (unsigned long long)run.bytes_in, (unsigned long long)run.chunks,
		        (unsigned long long)run.bai_bytes, run.read_s, run.up_s, run.inflate_s, run.walk_s, run.key_s, run.assemble_s, wall, acct.load());
	return rc;
}

extern "C" int al_index_bam(const char *bam, const char *bai, unsigned flags, int device, int n_threads, size_t piece_bytes, AlBaiStat *stat)
{
	const auto t_wall = std::chrono::steady_clock::now();
	if (stat) memset(stat, 0, sizeof(*stat));
	AlBaiRun run; size_t held = 0; bool on_device = false;
	const int rc = al_bai_index_file(bam, bai, (flags & AL_BAI_HOST) != 0, device, n_threads, piece_bytes, &run, &held, &on_device);
	if (stat) {
		stat->records = run.records; stat->unplaced = run.unplaced; stat->pieces = run.pieces; stat->bytes_in = run.bytes_in; stat->chunks = run.chunks; stat->bai_bytes = run.bai_bytes; stat->held = held;
		stat->read_s = run.read_s; stat->up_s = run.up_s; stat->inflate_s = run.inflate_s; stat->walk_s = run.walk_s; stat->key_s = run.key_s; stat->assemble_s = run.assemble_s;
		stat->wall_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_wall).count(); stat->on_device = on_device ? 1 : 0;
	}
	return rc;
}

// ---- test taps (airlift_amd/capi.py): al_bai_tap of al_bai.h with the twin and with the kernels ----------------------------------------------------------------------
static int bai_tap_out(int rc, const std::vector<uint8_t> &v, void *bai, size_t bai_cap, size_t *bai_n)
{
	*bai_n = rc == 0 ? v.size() : 0;
	if (rc) return rc;
	if (v.size() > bai_cap) return -3;
	memcpy(bai, v.data(), v.size());
	return 0;
}
extern "C" int al_dbg_bai_host(const void *bam, size_t n, const uint64_t *m_file, const uint64_t *m_stream, const uint32_t *m_isize, size_t n_mem, uint64_t file_end, size_t piece, void *bai, size_t bai_cap, size_t *bai_n)
{
	AlBaiHostBackend B; std::vector<uint8_t> v;
	return bai_tap_out(al_bai_tap(B, bam, n, m_file, m_stream, m_isize, n_mem, file_end, piece, v), v, bai, bai_cap, bai_n);
}
extern "C" int al_dbg_bai(int device, const void *bam, size_t n, const uint64_t *m_file, const uint64_t *m_stream, const uint32_t *m_isize, size_t n_mem, uint64_t file_end, size_t piece, void *bai, size_t bai_cap,
                          size_t *bai_n, size_t *held)
{
	*held = 0; *bai_n = 0;
	if (n >= ((size_t)1 << 31) - 65536) return -3;
	std::atomic<size_t> acct{0}; int rc; std::vector<uint8_t> v;
	{
		AlBaiDevBackend B; B.acct = &acct;
		if (B.open(device, 0, 0)) return -1;
		rc = al_bai_tap(B, bam, n, m_file, m_stream, m_isize, n_mem, file_end, piece, v);
	}
	*held = acct.load();
	return bai_tap_out(rc, v, bai, bai_cap, bai_n);
}

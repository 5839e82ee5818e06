// al_bam.h -- BAM record / BGZF writer used by the file-level driver (product code)
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <vector>
#include "al_internal.h"

struct AlDeflateDev;             // al_deflate.hip: the device compressor's stream and buffers
struct AlBgzf {                 // BGZF stream: bytes in, 64 KB blocks deflated on n_threads workers -- or, with AL_BAM_DEFLATE_DEVICE in the level, by the GPU -- written in order
	FILE *out; int level, n_threads;
	std::vector<char> buf; size_t cap;
	double t_deflate = 0;        // seconds spent compressing (wall time of the worker rounds), for the drivers' AL_TIMING lines
	// the device backend (--gpu-deflate): whole flushes go up, through k_deflate and come back as members; opened at the first flush
	bool dev_on = false; int dev_id = -1; AlDeflateDev *dev = nullptr;
	double t_kernel = 0, t_xfer = 0, t_host = 0; size_t n_blocks = 0, n_resident = 0, n_stored = 0, n_fallback = 0; bool told_nomem = false;   // kernel seconds (HIP events), copy seconds, host-twin seconds; blocks, blocks compressed where the batch lay, stored blocks, flushes the host twin took
	AlBgzf(FILE *o, int lvl, int nt, int device = -1) : out(o), level(lvl & 0xff), n_threads(nt > 1 ? nt : 1), cap((size_t)0xff00 * 64 * (size_t)(nt > 1 ? nt : 1)), dev_on((lvl & 0x100) != 0), dev_id(device) { buf.reserve(cap); }
	~AlBgzf();
	AlBgzf(const AlBgzf &) = delete; AlBgzf &operator=(const AlBgzf &) = delete;
	int write(const char *p, size_t n);
	int finish();                // flushes the tail and appends the EOF block
	int flush_all();             // everything written so far goes out as whole blocks (the tail as a short one), no EOF block: what follows may come from other writers
	// n bytes that lie in device memory (d_src, complete behind what stream st holds) as the stream's next bytes, compressed where they lie: the pending
	// carry (< 0xff00 bytes, host) goes up into the backend's seam buffer and is the first segment of the first block, the kernels run on st, the members
	// leave through the caller's two page-locked buffers of `piece` bytes (ev: their 'copied' events, of st's device) and are written, the tail
	// (< 0xff00 bytes) comes back as the new carry.  0: done; 1: not taken (backend off, fewer bytes than a block, or no device memory: the caller hands
	// the bytes to write() instead); -1: failed.
	int write_device(const char *d_src, size_t n, hipStream_t st, char *const ring[2], size_t piece, hipEvent_t const ev[2]);
	void timing_line(FILE *f, const char *who) const;   // the AL_TIMING line of the device backend
private:
	int flush_full();
	int deflate_dev(const char *p, size_t n);    // n bytes as members, compressed by the device backend, written
};
// al_deflate.hip
AlDeflateDev *al_deflate_dev_open(int device);
void al_deflate_dev_close(AlDeflateDev *d);
int al_deflate_dev_run(AlDeflateDev *d, const char *src, size_t n, int level, std::vector<unsigned char> &dst, size_t *n_stored, double *kernel_s, double *xfer_s);
int al_deflate_dev_run_resident(AlDeflateDev *d, hipStream_t st, const char *carry, size_t n_carry, const char *d_src, size_t n, int level, char *const ring[2], size_t piece, hipEvent_t const ev[2],
                                FILE *out, std::vector<char> &tail, size_t *n_stored, double *kernel_s, double *xfer_s);
int al_deflate_host_run(const char *src, size_t n, int level, int n_threads, std::vector<unsigned char> &dst, size_t *n_stored);


// BGZF input (--gpu-inflate; al_inflate.hip): the file's members inflated by k_inflate, a piece of the file at a time, and handed out as one byte stream.
// open(): true when the reader took the file; false with plain set when it is no BGZF file (gzip without the BC subfield, or "-"): the caller reads it as
// one gzip stream.  read(): n bytes, false at the end of the file or at an error -- failed() tells which, message() names the member's file offset and status.
struct AlBgzfInImpl;
struct AlBgzfIn {
	AlBgzfInImpl *p = nullptr; int device, n_threads; bool plain = false, host_backend = false, fell_back = false;
	AlBgzfIn(int device, int n_threads);
	~AlBgzfIn();
	AlBgzfIn(const AlBgzfIn &) = delete; AlBgzfIn &operator=(const AlBgzfIn &) = delete;
	bool open(const char *fn);
	bool read(void *dst, size_t n);
	bool failed() const;
	const char *message() const;
	void close();                 // stops the reader thread and releases the device and page-locked buffers
	void timing_line(FILE *f, double scan_s) const;   // the AL_TIMING line; scan_s: seconds the caller spent in its record loop, read() included
};

// n bytes of BAM records as a sequence of whole BGZF blocks (a record may span blocks), deflated on n_threads workers, appended to dst: a lane's
// share of a batch becomes a byte range that can be written at any offset of the output ("BGZF blocks are rank-local")
int al_bgzf_blocks(const char *src, size_t n, int level, int n_threads, std::vector<char> &dst);
extern const unsigned char AL_BGZF_EOF[28];
int al_bam_header(AlBgzf &z, const al_idx_t *mi, const char *rg, char *rg_id, bool sorted);
int al_write_bam_rec(std::vector<char> &out, const al_idx_t *mi, const char *qname, int l_seq, const char *seq, const char *qual,
                     int seg_idx, int reg_idx, int n_seg, const int *n_regss, const al_reg1_t *const *regss, const char *rg_id, int rep_len,
                     uint64_t *key, int *unmapped, int64_t opt_flag = 0, const char *tag = nullptr, int tag_len = 0);   // opt_flag, tag: as al_write_sam_ex
// stable sort permutation of n 64-bit keys, radix-sorted on the context's GPU (al_runtime.hip)
int al_sort_keys(al_ctx_t *c, const uint64_t *keys, uint32_t *perm, size_t n);

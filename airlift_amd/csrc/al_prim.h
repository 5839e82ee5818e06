// al_prim.h -- rocPRIM's two-call form (the size, then the work) written once, and the one scan that several files need
#pragma once
#include <rocprim/rocprim.hpp>
#include "al_runtime.h"

// call(nullptr, bytes) for the size of the temporary storage, tmp grown to it (+ 16), call(tmp.p, bytes) for the work.  0; AL_ERR_NOMEM when tmp cannot grow
// (DevBuf::ensure has said so and set al_nomem_flag); -1 on a HIP error, reported at the caller's file and line: as AL_HIP_CHECK does, or under `tag`.
template <class F>
static inline int al_prim_run(DevBuf<uint8_t> &tmp, F call, const char *tag = nullptr, int line = __builtin_LINE(), const char *file = __builtin_FILE())
{
	size_t bytes = 0;
	hipError_t e = call((void *)nullptr, bytes);
	if (e == hipSuccess) {
		if (tmp.ensure(bytes + 16, false, 0, line, file)) return AL_ERR_NOMEM;
		e = call((void *)tmp.p, bytes);
	}
	if (e == hipSuccess) return 0;
	if (tag) fprintf(stderr, "[airlift] %s: rocPRIM at %s:%d: %s\n", tag, file, line, hipGetErrorString(e));
	else fprintf(stderr, "[airlift] HIP error %s at %s:%d: %s\n", hipGetErrorName(e), file, line, hipGetErrorString(e));
	return -1;
}

struct AlCastU64 { __host__ __device__ uint64_t operator()(const uint32_t &v) const { return (uint64_t)v; } };
// out[0, n) = the exclusive sums of in[0, n), as uint64_t (a template, so that only the files that call it carry the scan's kernels in their code objects)
template <class Out = uint64_t>
static inline int al_prim_scan_u32_u64(DevBuf<uint8_t> &tmp, const uint32_t *in, Out *out, size_t n, hipStream_t s, int line = __builtin_LINE(), const char *file = __builtin_FILE())
{
	auto it = rocprim::make_transform_iterator(in, AlCastU64());
	return al_prim_run(tmp, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, it, out, (uint64_t)0, n, rocprim::plus<uint64_t>(), s); }, nullptr, line, file);
}

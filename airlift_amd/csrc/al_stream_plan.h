// al_stream_plan.h -- which physical stream each stream role of a mapping context runs on (host only: no HIP include, so that a plain
// C++ program can include it -- tests/csrc/stream_plan_main.cpp)
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <assert.h>

// The ten stream roles of a mapping context (al_ctx_s, al_runtime.h), in the order their streams are created.
enum AlRole {
	AL_ROLE_MAIN = 0,                             // the pipeline itself
	AL_ROLE_SIDE,                                 // equal-x heap merges beside the chaining; k_ext_prep_wave and k_align beside the DP classes
	AL_ROLE_AUX0, AL_ROLE_AUX1, AL_ROLE_AUX2,     // the other heap merge classes; the k_regs_select / k_regs_heavy classes; DP classes of a small batch
	AL_ROLE_OVL0,                                 // the run sort of the giant fragments beside the block sorts (the host waits for its set-up)
	AL_ROLE_OVL1, AL_ROLE_OVL2,                   // the lane chaining kernels of the small fragments, the classes in turn
	AL_ROLE_SPEC, AL_ROLE_SPEC2,                  // the giant-fragment merges made ahead of the re-chain pass (the host waits for them at the next batch's start)
	AL_ROLE_N
};

// Number of physical streams of a context: AL_STREAMS (1 ... 10) if set, else min(10, GPU_MAX_HW_QUEUES) with the variable as the environment has
// it, else HIP's default of 4 hardware queues.  *source: 0 AL_STREAMS, 1 the environment's queue count, 2 the default.
static inline int al_stream_count(const char *al_streams, const char *hw_queues, int *source)
{
	int n = al_streams ? atoi(al_streams) : 0;
	if (n >= 1) { if (source) *source = 0; return n < AL_ROLE_N ? n : (int)AL_ROLE_N; }
	n = hw_queues ? atoi(hw_queues) : 0;
	if (n >= 1) { if (source) *source = 1; return n < AL_ROLE_N ? n : (int)AL_ROLE_N; }
	if (source) *source = 2;
	return 4;
}

// Roles that never share a stream when there are four or more (DESIGN.md 4 has the timelines behind them).
struct AlRolePair { uint8_t a, b; };
static const AlRolePair AL_NEVER_TOGETHER[] = {
	// The merges made ahead are launched right after seeding and run for milliseconds, up to the re-chain pass.  Behind them would wait:
	// ovl0's set-up kernels, which the HOST waits for in mid-step while it launches nothing on main;
	{AL_ROLE_OVL0, AL_ROLE_SPEC}, {AL_ROLE_OVL0, AL_ROLE_SPEC2},
	// the lane chaining, which main joins before the tile kernel;
	{AL_ROLE_OVL1, AL_ROLE_SPEC}, {AL_ROLE_OVL1, AL_ROLE_SPEC2}, {AL_ROLE_OVL2, AL_ROLE_SPEC}, {AL_ROLE_OVL2, AL_ROLE_SPEC2},
	// the first pass's equal-x heap merges (side, aux0, aux2), which main joins before the re-chain pass.
	{AL_ROLE_SIDE, AL_ROLE_SPEC}, {AL_ROLE_SIDE, AL_ROLE_SPEC2}, {AL_ROLE_AUX0, AL_ROLE_SPEC}, {AL_ROLE_AUX0, AL_ROLE_SPEC2}, {AL_ROLE_AUX2, AL_ROLE_SPEC}, {AL_ROLE_AUX2, AL_ROLE_SPEC2},
	// The run sort of the giant fragments (one 18 ms kernel) starts before the lane chaining, and main joins both.
	{AL_ROLE_OVL0, AL_ROLE_OVL1}, {AL_ROLE_OVL0, AL_ROLE_OVL2},
	// k_align runs on side to the end of the DP classes; k_ext_finish_wave (aux0) and the thin 22-block DP class (aux1) must not queue behind it.
	{AL_ROLE_SIDE, AL_ROLE_AUX0}, {AL_ROLE_SIDE, AL_ROLE_AUX1},
	// The long classes of k_regs_select and k_regs_heavy (aux0: 6.9 and 2.4 ms, aux1: 4.2 and 3.2 ms of a 1 M-pair batch) beside each other.
	{AL_ROLE_AUX0, AL_ROLE_AUX1},
};
static const int AL_N_NEVER_TOGETHER = (int)(sizeof(AL_NEVER_TOGETHER) / sizeof(AL_NEVER_TOGETHER[0]));

// map[role] = physical stream, 0 ... n_phys - 1, for n_phys = 1 ... 10 (clamped).  Physical 0 is main's and, from two streams on, nobody else's.
//   1   everything in main's order: the correctness baseline
//   2   everything that ran beside main on one stream
//   3   the four-stream plan with its third stream (the long thin tails) folded onto the second
//   4   the default of a HIP process:
//         1: ovl0, then side and aux2 -- the run sort is over when the heap merges start, and nothing of an earlier stage is left on it when the host
//            waits for ovl0's set-up; side's k_regs_heavy class is the shortest, so aux2's (and k_regs) follow it
//         2: ovl1 + ovl2, then aux0 -- the lane chaining classes one after the other still end (15 ms) before the block sorts on main do (21 ms)
//         3: spec + spec2, then aux1 -- the merges made ahead need not be over before the re-chain pass's merge stage; aux1 has no kernel before the regs stage
//   5 ... 9   unfold: aux2 (k_regs_heavy: five classes and k_regs on four streams is the one stage that is longer than with a stream each) | ovl2 | ovl0 | ovl1 | spec
//   10  a stream per role: the arrangement the fork / join code was written for
static inline void al_stream_plan(int n_phys, uint8_t map[AL_ROLE_N])
{
	static const uint8_t plan[10][AL_ROLE_N] = {
		//       main side aux0 aux1 aux2 ovl0 ovl1 ovl2 spec spec2
		/*  1 */ {0,  0,   0,   0,   0,   0,   0,   0,   0,   0},
		/*  2 */ {0,  1,   1,   1,   1,   1,   1,   1,   1,   1},
		/*  3 */ {0,  1,   2,   2,   1,   1,   2,   2,   2,   2},
		/*  4 */ {0,  1,   2,   3,   1,   1,   2,   2,   3,   3},
		/*  5 */ {0,  1,   2,   3,   4,   1,   2,   2,   3,   3},
		/*  6 */ {0,  1,   2,   3,   4,   1,   2,   5,   3,   3},
		/*  7 */ {0,  1,   2,   3,   4,   5,   2,   6,   3,   3},
		/*  8 */ {0,  1,   2,   3,   4,   5,   6,   7,   3,   3},
		/*  9 */ {0,  1,   2,   3,   4,   5,   6,   7,   8,   8},
		/* 10 */ {0,  1,   2,   3,   4,   5,   6,   7,   8,   9},
	};
	if (n_phys < 1) n_phys = 1;
	if (n_phys > AL_ROLE_N) n_phys = AL_ROLE_N;
	for (int r = 0; r < AL_ROLE_N; ++r) { map[r] = plan[n_phys - 1][r]; assert(map[r] < n_phys); }
	assert(map[AL_ROLE_MAIN] == 0);
	if (n_phys >= 4) for (int k = 0; k < AL_N_NEVER_TOGETHER; ++k) assert(map[AL_NEVER_TOGETHER[k].a] != map[AL_NEVER_TOGETHER[k].b]);
}

// AL_STREAM_MAP="0,1,2,3,1,1,2,2,3,3" (experiments: a map given role by role, in AlRole's order): the number of streams it uses, or 0 when it is not
// ten numbers with main alone on 0 and every stream up to the largest in use.
static inline int al_stream_map_parse(const char *s, uint8_t map[AL_ROLE_N])
{
	if (!s) return 0;
	int n = 0; unsigned used = 0;
	for (int r = 0; r < AL_ROLE_N; ++r) {
		char *e = nullptr; const long v = strtol(s, &e, 10);
		if (e == s || v < 0 || v >= AL_ROLE_N || (r + 1 < AL_ROLE_N ? *e != ',' : *e != 0)) return 0;
		map[r] = (uint8_t)v; used |= 1u << v; if (v + 1 > n) n = (int)v + 1;
		s = e + 1;
	}
	if (used != (1u << n) - 1u || map[AL_ROLE_MAIN] != 0) return 0;
	for (int r = 1; r < AL_ROLE_N; ++r) if (n > 1 && map[r] == 0) return 0;
	return n;
}

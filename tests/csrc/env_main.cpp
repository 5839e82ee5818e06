// env_main.cpp -- the table of environment variables (airlift_amd/csrc/al_env.h) as a stand-alone host program: it includes nothing but that header and
// prints every field of al_env() and of al_env_ctx(), then what the per-call functions return, as name=value lines ("unset" for an absent optional or
// text).  `make san-env` builds it with AddressSanitizer + UBSan; tests/test_env_cpu.py runs it under one environment per case.
#include <stdio.h>
#include "al_env.h"

static void text(const char *n, const char *v) { if (v) printf("%s=%s\n", n, v); else printf("%s=unset\n", n); }
static void opt_i(const char *n, const std::optional<int> &v) { if (v) printf("%s=%d\n", n, *v); else printf("%s=unset\n", n); }
static void opt_d(const char *n, const std::optional<double> &v) { if (v) printf("%s=%.17g\n", n, *v); else printf("%s=unset\n", n); }

int main()
{
	const AlEnv &e = al_env();
	printf("trace=%d\n", (int)e.trace);
	printf("timing=%d\n", (int)e.timing);
	printf("timing_nonzero=%d\n", (int)e.timing_nonzero);
	printf("trace_alloc=%d\n", (int)e.trace_alloc);
	printf("serial_parse=%d\n", (int)e.serial_parse);
	opt_i("idx_threads", e.idx_threads);
	printf("pg_plain=%d\n", (int)e.pg_plain);
	printf("no_rccl=%d\n", (int)e.no_rccl);
	printf("host_io=%d\n", (int)e.host_io);
	printf("host_index=%d\n", (int)e.host_index);
	printf("no_reserve=%d\n", (int)e.no_reserve);
	opt_d("reserve_kb_per_read", e.reserve_kb_per_read);
	printf("pool_chunk_gb=%.17g\n", e.pool_chunk_gb);
	printf("hbm_margin_mb=%d\n", (int)e.hbm_margin_mb);
	printf("rank_timeout=%.17g\n", e.rank_timeout);
	printf("no_fast_exit=%d\n", (int)e.no_fast_exit);
	opt_i("dbg_frag", e.dbg_frag);
	text("gpu_max_hw_queues", e.gpu_max_hw_queues);
	opt_i("slots", e.slots);
	opt_i("ctxs", e.ctxs);
	printf("piece_mb=%d\n", (int)e.piece_mb);
	printf("out_piece_mb=%d\n", (int)e.out_piece_mb);
	printf("inflate_piece_kb=%d\n", (int)e.inflate_piece_kb);
	opt_i("batch_reads", e.batch_reads);
	printf("long_batch=%.17g\n", e.long_batch);
	printf("long_batch_big_from=%.17g\n", e.long_batch_big_from);
	opt_i("probe_reads", e.probe_reads);
	opt_i("probe_mult", e.probe_mult);
	printf("two_probes=%d\n", (int)e.two_probes);
	printf("alloc_gbs=%.17g\n", e.alloc_gbs);
	printf("batch_ms=%.17g\n", e.batch_ms);
	text("streams", e.streams);
	text("stream_map", e.stream_map);
	text("test_poison", e.test_poison);
	text("test_poison_only", e.test_poison_only);
	printf("test_poison_log=%d\n", (int)e.test_poison_log);
	printf("test_guard=%d\n", (int)e.test_guard);
	text("test_sort_blk", e.test_sort_blk);
	text("test_sort_big", e.test_sort_big);
	text("test_big_chunk", e.test_big_chunk);
	text("test_run", e.test_run);
	text("test_nomem_above", e.test_nomem_above);
	text("test_scrub", e.test_scrub);
	printf("test_deflate_nomem=%d\n", (int)e.test_deflate_nomem);
	printf("test_inflate_nomem=%d\n", (int)e.test_inflate_nomem);
	printf("test_inflate_host=%d\n", (int)e.test_inflate_host);
	printf("test_tile_all=%d\n", (int)e.test_tile_all);
	printf("test_tile_fb=%d\n", (int)e.test_tile_fb);
	opt_i("test_seg_big", e.test_seg_big);
	printf("test_heap_wave=%d\n", (int)e.test_heap_wave);
	printf("chain_coop=%d\n", (int)e.chain_coop);
	printf("chain_ovl=%d\n", (int)e.chain_ovl);
	printf("chain_ovl2=%d\n", (int)e.chain_ovl2);
	printf("chain_wave_max=%u\n", e.chain_wave_max);
	opt_i("prep_heavy", e.prep_heavy);
	printf("fin_heavy=%d\n", (int)e.fin_heavy);
	printf("regs_split=%d\n", (int)e.regs_split);
	printf("heap_old=%d\n", (int)e.heap_old);
	printf("spec_merge=%d\n", (int)e.spec_merge);
	opt_i("spec_min", e.spec_min);
	printf("dp_pk=%d\n", (int)e.dp_pk);
	printf("dp_pk32=%d\n", (int)e.dp_pk32);
	printf("big_merge=%d\n", (int)e.big_merge);
	printf("order_block=%d\n", (int)e.order_block);
	printf("dp_conc=%lld\n", e.dp_conc);
	printf("side_prio=%d\n", (int)e.side_prio);
	printf("dp_no_split=%d\n", (int)e.dp_no_split);
	printf("cap4=%d\n", (int)e.cap4);
	printf("cap8=%d\n", (int)e.cap8);
	printf("cap22=%d\n", (int)e.cap22);
	printf("grow_div=%d\n", (int)e.grow_div);
	const AlEnvCtx c = al_env_ctx();
	printf("ctx.dbg=%d\n", (int)c.dbg);
	printf("ctx.dbg2=%d\n", (int)c.dbg2);
	printf("ctx.dp_exit=%d\n", (int)c.dp_exit);
	printf("ctx.dp_exit_stride=%d\n", (int)c.dp_exit_stride);
	text("ctx.dp_exit_stride_refused", c.dp_exit_stride_refused);
	opt_i("call.rank", al_env_rank());
	opt_i("call.world_size", al_env_world_size());
	printf("call.pick_device(-1,8)=%d\n", al_env_pick_device(-1, 8));
	printf("call.pick_device(-1,8,11)=%d\n", al_env_pick_device(-1, 8, 11));
	printf("call.pick_device(-1,0,11)=%d\n", al_env_pick_device(-1, 0, 11));
	printf("call.pick_device(5,8)=%d\n", al_env_pick_device(5, 8));
	text("call.run_id", al_env_run_id());
	printf("call.run_id_vouched=%d\n", (int)al_env_run_id_vouched());
	text("call.tmpdir", al_env_tmpdir());
	printf("call.sort_mem=%llu\n", (unsigned long long)al_env_sort_mem());
	printf("call.auto_batch=%d\n", (int)al_env_auto_batch());
	printf("call.no_pwrite=%d\n", (int)al_env_no_pwrite());
	printf("call.rank_batch=%lld\n", al_env_rank_batch());
	return 0;
}

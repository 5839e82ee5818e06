#!/bin/bash
# Profiling recipe (run on the GPU box through gpurun): kernel trace + stats, then HBM PMC passes (separate runs).
# usage: tools/prof.sh <tag> [bench args...]      (default workload: bench.py's default, C4)
# Every pass runs under a time limit of its own (PROF_STEP_TIMEOUT seconds, default 300) and nothing is started after a pass that failed.
set -u
TAG=${1:-r02}; shift || true
REPO=${GRAFT_REPO_ROOT:-/root/repo}
OUT=$REPO/gpurun_out/prof_$TAG
mkdir -p $OUT
export AL_REF_CACHE=/tmp/alcache
cd /tmp && export TMPDIR=/tmp
T="timeout -k 10 ${PROF_STEP_TIMEOUT:-300}"
ARGS="--no-cpu-baseline --f2f-pairs 0 --steps 3 --warmup 1 $*"
$T rocprofv3 --kernel-trace --stats -d $OUT/trace --output-format csv -- python3 $REPO/bench.py $ARGS > $OUT/bench_trace.json 2> $OUT/trace.err &&
$T rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $OUT/pmc_fetch --output-format csv -- python3 $REPO/bench.py $ARGS > $OUT/bench_fetch.json 2> $OUT/fetch.err &&
$T rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $OUT/pmc_write --output-format csv -- python3 $REPO/bench.py $ARGS > $OUT/bench_write.json 2> $OUT/write.err &&
$T rocprofv3 --pmc SQ_INSTS_VALU --kernel-trace -d $OUT/pmc_valu --output-format csv -- python3 $REPO/bench.py $ARGS > $OUT/bench_valu.json 2> $OUT/valu.err &&
python3 $REPO/tools/prof_summary.py $OUT > $OUT/summary.md 2>&1
RC=$?
# keep only small files for the merge back (<= 64 MiB)
find $OUT -name "*.csv" -size +6M -delete
ls -la $OUT | head -20; tail -n 2 $OUT/*.err | cut -c1-200
exit $RC

#!/bin/bash
# the round's bench lines: tools/r6_bench_all.sh <tag> <dir>  ->  <dir>/<tag>_bench_{c2,c3,c5,c4_default}.json (--full: C2 / C3 / C5 with their CPU comparator, no file-to-file leg; C4 = the default workload with every leg)
tag=${1:-r06b}; out=${2:?output directory}; mkdir -p "$out"
export AL_REF_CACHE=/tmp/alcache TMPDIR=/tmp
for c in c2 c3 c5; do
  p=1000000; [ $c = c5 ] && p=500000
  timeout 500 python bench.py --full --config $c --pairs $p --steps 10 --warmup 3 --f2f-pairs 0 > "$out/${tag}_bench_$c.json" 2> "$out/${tag}_bench_$c.err"; tail -c 300 "$out/${tag}_bench_$c.err"
done
timeout 900 python bench.py --full > "$out/${tag}_bench_c4_default.json" 2> "$out/${tag}_bench_c4.err"; tail -c 300 "$out/${tag}_bench_c4.err"
python - <<PY
import json
for c in ("c2","c3","c5","c4_default"):
    try:
        d=json.loads(open("$out/${tag}_bench_%s.json"%c).read().strip().splitlines()[-1]); print(c, round(d["ms_per_step"],2), round(d["value"]), d.get("parity_sample"), (d.get("file_to_file") or {}).get("reads_per_s"), (d.get("cpu_baseline") or {}).get("value"))
    except Exception as e: print(c, "failed", e)
PY

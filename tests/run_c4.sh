# C4 (batch of clips) through bench.py --full; summary on stdout, JSON under the output directory (default bench_out/)
OUT=${1:-bench_out}; mkdir -p $OUT
timeout -k 10 400 python bench.py --config C4 --steps 10 --warmup 2 --full > $OUT/bench_c4.json 2> $OUT/bench_c4.err || { tail -5 $OUT/bench_c4.err; exit 1; }
python3 - "$OUT" <<'PY'
import json, sys
d = json.load(open(sys.argv[1] + "/bench_c4.json"))
print(d["value"], d["ms_per_step"], d["config"]["workload"], d["roofline"]["kernel"], d["roofline"]["frac"])
print(d.get("end_to_end")); print(d.get("cpu_baseline"), d.get("speedup_vs_cpu")); print(d["stage_ms"])
PY

#!/bin/bash
# what the driver runs at round end, in one call: the -m gpu suite, smoke(), the full bench line (bench.py --full)
out=${1:?usage: tools/r6_final_check.sh <output directory>}
mkdir -p "$out"
timeout -k 10 1000 python -m pytest tests -m gpu -q > "$out/t_final.log" 2>&1
grep -E "^FAILED|^ERROR|passed|failed" "$out/t_final.log" | cut -c1-250
python __graft_entry__.py smoke 2>&1 | tail -2 | cut -c1-300
python bench.py --full > "$out/bench_final.json" 2> "$out/bench_final.err"; python -c "
import json; d=json.load(open('$out/bench_final.json')); print(d['value'], d['ms_per_step'], d['roofline']['frac'], d['roofline'].get('mfma_busy_3x3'), d['cpu_baseline']['value'], (d.get('range') or {}).get('exceeded'))"

#!/bin/bash
# The two layouts of the wide main pass from one build (profiles/wide_side_by_side/side_by_side_ab.txt): N alternating
# bench.py runs per arm, then FETCH_SIZE + GRBM_GUI_ACTIVE of the main-pass launches in a counter run of their own per arm.
# Usage: scripts/wide_layout_ab.sh OUT_DIR [RUNS] [extra bench.py arguments, e.g. --rows 1250000]
set -e -o pipefail
OUT=${1:?output directory}; RUNS=${2:-5}; shift; shift || true
mkdir -p "$OUT"
for i in $(seq 1 "$RUNS"); do
    FSGPU_WIDE_LAYOUT=sequential timeout -k 10 300 python bench.py --gpus 1 --steps 100 --warmup 10 "$@" 2> /dev/null | grep '^{' >> "$OUT/bench_sequential.jsonl"
    timeout -k 10 300 python bench.py --gpus 1 --steps 100 --warmup 10 "$@" 2> /dev/null | grep '^{' >> "$OUT/bench_side_by_side.jsonl"
done
python - "$OUT" <<'PY'
import json, statistics, sys
for arm in ("sequential", "side_by_side"):
    ms = [json.loads(l)["ms_per_step"] for l in open(f"{sys.argv[1]}/bench_{arm}.jsonl")]
    print(f"{arm:13s} ms per step: " + " ".join(f"{m:.4f}" for m in ms) + f"   median {statistics.median(ms):.4f}   max - min {max(ms) - min(ms):.4f}")
PY
for arm in sequential side_by_side; do
    if [ $arm = sequential ]; then export FSGPU_WIDE_LAYOUT=sequential; else unset FSGPU_WIDE_LAYOUT; fi
    timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE GRBM_GUI_ACTIVE --output-format csv -d "$OUT/pmc_$arm" -o bench -- \
        python bench.py --gpus 1 --steps 4 --warmup 1 "$@" > "$OUT/pmc_$arm.log" 2>&1
    python scripts/pmc_summary.py "$OUT/pmc_$arm" "$OUT/pmc_$arm.json" | grep scan_wide_kernel | sed "s/^/$arm /"
done

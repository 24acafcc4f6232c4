#!/bin/bash
# profiles/time_update.py on the GPU: the timings, then (a run of its own) the kernels' times.
# Each step under its own time limit, chained: a step that fails, faults or runs out of time
# ends the script.  Usage: profiles/time_update.sh [output directory]
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${1:-profiles/update_values}
mkdir -p "$OUT"
timeout -k 10 600 python profiles/time_update.py --out "$OUT/time_update.json" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace" -o update -- \
    python profiles/time_update.py --what device --reps 3 > "$OUT/trace_run.txt" 2>&1 &&
grep -h -E "k_value_scatter|k_shell_rebuild|k_shell_rects|k_shell_init|k_max_opacities" \
    "$OUT"/trace/update_kernel_stats.csv | tee "$OUT/kernel_stats.txt"

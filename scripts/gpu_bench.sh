#!/bin/bash
# microbench detail + the full bench record + rocprof kernel stats of the headline-only command.
# Usage (on an MI355X): bash scripts/gpu_bench.sh [tag] [output directory, default bench_out/]
set -o pipefail
TAG=${1:-r01}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${2:-$R/bench_out}
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd)
cd "$R"
python - <<'PY' 2>&1 | tee "$OUT/microbench_${TAG}.log"
import __graft_entry__ as ge
ge.build()
from nowcastautogp_amd import _lib
c = _lib.Context(0)
for bpc in (1, 2, 4):
    print(c.microbench_mfma_f64_detail(40000, bpc))
w, cp = c.microbench_hbm(1 << 31)
print(f"hbm write {w:.0f} GB/s  copy {cp:.0f} GB/s")
PY
python bench.py --full --steps 2 --warmup 1 2>"$OUT/bench_${TAG}.err" | tee "$OUT/bench_${TAG}.json"
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_${TAG}" -- python3 "$R/bench.py" --steps 1 --warmup 0 --headline-only > "$OUT/prof_${TAG}.log" 2>&1
cd "$R"
find "$OUT/prof_${TAG}" -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} "$OUT/kernel_stats_${TAG}.csv"
head -20 "$OUT/kernel_stats_${TAG}.csv"

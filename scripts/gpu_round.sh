#!/bin/bash
# One GPU-box visit: parity tests, smoke, bench, rocprofv3 kernel stats.  Usage (from the repo root on the box):
#   bash scripts/gpu_round.sh [tests|notests] [tag] [output dir, default runs/<tag>]
R=${GRAFT_REPO_ROOT:-$(pwd)}
TAG=${2:-r01}
O=${3:-$R/runs/$TAG}
mkdir -p $O
cd $R
if [ "${1:-tests}" = "tests" ]; then
  (timeout 1500 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider 2>&1 | tail -120) > $O/pytest_gpu.log 2>&1
  tail -5 $O/pytest_gpu.log
  (timeout 600 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -20) > $O/smoke.log 2>&1
  tail -3 $O/smoke.log
fi
(timeout 900 python bench.py --full 2>&1 | tail -5) > $O/bench_${TAG}.log 2>&1
tail -2 $O/bench_${TAG}.log
(timeout 600 python bench.py --full --model xlnet --cpu-steps 1 2>&1 | tail -2) > $O/bench_xlnet_${TAG}.log 2>&1
tail -1 $O/bench_xlnet_${TAG}.log | cut -c1-400
cd /tmp && export TMPDIR=/tmp
rm -rf /tmp/prof && mkdir -p /tmp/prof
(timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof -o bench -- python $R/bench.py --full --steps 10 --warmup 3 --cpu-baseline 0 2>&1 | tail -3) > $O/rocprof_${TAG}.log 2>&1
find /tmp/prof -type f | head
for f in $(find /tmp/prof -name "*kernel_stats.csv"); do cp $f $O/bench_kernel_stats_${TAG}.csv; done
head -40 $O/bench_kernel_stats_${TAG}.csv

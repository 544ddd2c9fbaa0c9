#!/bin/bash
# Round-end evidence: full bench line + rocprofv3 kernel stats of the same command (GPU box).
#   bash tools/round_profile.sh <tag> [dir]   -> <dir>/<tag>_bench_line.json, <dir>/<tag>_kernel_stats.csv
#   (dir: profile_out/ at the repository root unless given; copy what is kept to profiles/)
TAG=${1:-rX}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${2:-$R/profile_out}; mkdir -p $OUT; OUT=$(cd $OUT && pwd)
cd $R && python bench.py --full --steps 8 --warmup 3 > $OUT/${TAG}_bench.log 2>&1
tail -1 $OUT/${TAG}_bench.log > $OUT/${TAG}_bench_line.json
cd /tmp && export TMPDIR=/tmp
rm -rf /tmp/prof_$TAG
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_$TAG -- python $R/bench.py --full --steps 8 --warmup 3 > $OUT/${TAG}_prof.log 2>&1
f=$(find /tmp/prof_$TAG -name '*kernel_stats.csv' | head -1)
cp "$f" $OUT/${TAG}_kernel_stats.csv
head -8 $OUT/${TAG}_kernel_stats.csv | cut -c1-160
cat $OUT/${TAG}_bench_line.json | cut -c1-900

# usage: bash tools/prof_kernel_stats.sh <output dir>   -> <output dir>/prof_r01b_kernel_stats.csv
ROOT=$(cd "$(dirname "$0")/.." && pwd); mkdir -p "$1"; OUT=$(cd "$1" && pwd)
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_r01b -- python $ROOT/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --batched-songs 0 --profile-steps 1 > $OUT/prof_r01b.log 2>&1
cd $OUT; find prof_r01b -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} prof_r01b_kernel_stats.csv; tail -2 prof_r01b.log | cut -c1-300; find prof_r01b -name "*kernel_trace.csv" -delete; ls prof_r01b/*

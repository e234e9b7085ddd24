# Step time against kernel time in ONE run (tag $1): bench.py under a rocprofv3
# kernel trace, then tools/step_gap.py over the timed CG passes. Outputs under
# $OUT (default prof_out/).
export TMPDIR=/tmp
T=${1:-cur}
shift
OUT=${OUT:-prof_out}
mkdir -p $OUT
rm -rf $OUT/gap_$T
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/gap_$T -o run -- python3 bench.py --steps 200 --warmup 20 --applies 20 --full --no-cpu-baseline --no-weak "$@" > $OUT/gap_$T.log 2>&1 &&
python3 tools/step_gap.py $(find $OUT/gap_$T -name "*kernel_trace.csv" | head -1) --last 200 >> $OUT/gap_$T.log 2>&1

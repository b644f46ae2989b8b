set -u
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/wprof -o run -- python3 -u bench.py --full --no-cpu --sim-n 0 --sim5-n 0 --no-merge --steps 3 --warmup 1 > $OUT/wprof.json 2> $OUT/wprof.err
find $OUT/wprof -name "*kernel_stats.csv" -exec cp {} $OUT/wprof_stats.csv \;

OUT=${OUT:-bench_out}/$1
RP_AMD_LIB=$PWD/ab/librpamd_wprof.so timeout -k 10 200 python -u bench.py --full --no-cpu --sim-n 0 --sim5-n 0 --no-merge --steps 2 --warmup 1 --batch-log2 20 > $OUT/wp.json 2> $OUT/wp.err; grep "wire wave cycles" $OUT/wp.err | tail -1

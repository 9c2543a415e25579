# bench (d4ic + grid, c5) and rocprofv3 kernel-trace summary of the d4ic bench
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 300 python -u bench.py --full > $OUT/bench.log 2>&1 && \
timeout -k 10 300 python -u bench.py --full --config c5 --no-cpu-baseline --steps 50 --warmup 5 --replicas 1 > $OUT/bench_c5.log 2>&1 && \
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/kt -o run -- python bench.py --full --no-cpu-baseline --steps 300 --warmup 30 --replicas 1 > $OUT/kt.log 2>&1

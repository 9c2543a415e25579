cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/kt_c5 -o run -- python bench.py --full --config c5 --no-cpu-baseline --steps 20 --warmup 3 --replicas 1 --no-kernel-times > $OUT/kt_c5.log 2>&1

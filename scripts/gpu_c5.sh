cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > $OUT/pytest_gpu.log 2>&1
echo "pytest rc=$?"
for c in d4ic c5; do timeout -k 10 200 python -u bench.py --full --config $c --no-cpu-baseline --steps 100 --warmup 10 > $OUT/bench_$c.log 2>&1 || { echo "bench $c failed"; break; }; done

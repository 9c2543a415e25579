cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 400 python -u -m pytest tests/test_gpu_parity.py -m gpu -v --timeout 200 --timeout-method thread -k "three_phases or stress" > $OUT/pytest_mfma.log 2>&1
echo "pytest rc=$?"
timeout -k 10 200 python -u bench.py --full --config c5 --no-cpu-baseline --steps 50 --warmup 5 --replicas 1 > $OUT/bench_c5.log 2>&1

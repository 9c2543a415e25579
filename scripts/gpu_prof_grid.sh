#!/bin/bash
# Kernel trace of the packed grid-search run (R = 32 replicas per launch).
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/kt_grid -o run -- python bench.py --full --no-cpu-baseline --no-kernel-times --steps 10 --warmup 2 --replicas 32 --grid-steps 50 > $OUT/kt_grid.log 2>&1

#!/bin/bash
# Round-end rehearsal on one box: the full -m gpu suite, smoke(), and the N-rank bench path with 2 ranks sharing the
# GPU (gloo; the driver's multi-GPU run uses RCCL, one rank per GPU).  Stops at the first failing step.
set -u
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread -rf > $OUT/pytest_all.log 2>&1
rc=$?; tail -4 $OUT/pytest_all.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { tail -5 $OUT/smoke.log; exit 1; }
tail -1 $OUT/smoke.log
RRTMGPNN_DIST_BACKEND=gloo timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29531 bench.py --gpus 2 --steps 20 --warmup 3 --full --no-cpu-baseline > $OUT/bench_n2.json 2> $OUT/bench_n2.err || { tail -5 $OUT/bench_n2.err; exit 1; }
head -c 600 $OUT/bench_n2.json; echo

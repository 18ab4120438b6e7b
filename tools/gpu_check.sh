#!/bin/bash
# One gpurun call: GPU tests, smoke, bench, rocprofv3 kernel-trace stats of the bench.
# Output under gpurun_out/$TAG.
set -e
cd "$GRAFT_REPO_ROOT"
export TMPDIR=/tmp
TAG=${TAG:-r01}
O=gpurun_out/$TAG
mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $O/pytest_gpu.log 2>&1 || { tail -30 $O/pytest_gpu.log; exit 1; }
tail -2 $O/pytest_gpu.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1
tail -1 $O/smoke.log
timeout -k 10 400 python bench.py --full > $O/bench.json 2> $O/bench.err
cat $O/bench.json
BENCH="bench.py --steps 20 --warmup 3 --cpu-seconds 0 --throughput-batch 0 --extras 0"
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/kt -o kt -- python3 $BENCH > $O/kt.log 2>&1
echo done

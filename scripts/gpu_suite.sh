#!/bin/bash
# the whole GPU suite + smoke (+ optionally the `--full` bench line) into OUT_DIR (default evidence/): bash scripts/gpu_suite.sh TAG [bench]
export TMPDIR=/tmp
O=${OUT_DIR:-evidence}; mkdir -p "$O"
T=${1:-r05}
timeout 1500 python -m pytest tests -m gpu -q --no-header -p no:cacheprovider --timeout=900 --timeout-method=thread --durations=8 -x 2>&1 | tail -n 40 > $O/${T}_pytest_gpu.txt; tail -n 25 $O/${T}_pytest_gpu.txt
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -n 1
if [ "$2" = "bench" ]; then timeout 400 python bench.py --full 2>/dev/null | tail -n 1 > $O/${T}_bench_default.json; cut -c1-400 $O/${T}_bench_default.json; fi

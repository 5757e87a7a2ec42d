#!/bin/bash
# Closing run of a round: the full GPU suite, smoke, then the evidence set (into OUT_DIR, default evidence/) in the order of its importance (a run that is cut short keeps what came first): the
# `--full` bench line, kernel stats of the same command, the eight-strip runs of BASELINE.json configs[3] / [4] with segment traces and projections, one-step timeline, CRCs of the
# native harness, config 3's kernel stats, SQ / FETCH / WRITE counter passes (each --pmc pass on its own, no trace domains).
export TMPDIR=/tmp
O=$(realpath -m "${OUT_DIR:-evidence}"); mkdir -p "$O"
R=$(cd "$(dirname "$0")/.." && pwd)
T=${1:-r06z}
[ "$2" = "nopytest" ] || timeout 1700 python -m pytest tests -m gpu -q --no-header -p no:cacheprovider --timeout=1200 --timeout-method=thread --durations=8 2>&1 | tail -n 20 > $O/${T}_pytest_gpu.txt; tail -n 14 $O/${T}_pytest_gpu.txt
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -n 2
timeout 600 python bench.py --full > $O/${T}_bench_default.log 2>&1; tail -n 1 $O/${T}_bench_default.log > $O/${T}_bench_default.json; cut -c1-700 $O/${T}_bench_default.json
(cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$T -o r -- python $R/bench.py --full --cpu-sample 0 --no-extras > $O/prof_$T.log 2>&1)
find $O/prof_$T -name "*kernel_stats.csv" | head -n 1 | xargs -I{} cp {} $O/${T}_kernel_stats_16384_default_bench.csv
rm -rf $O/prof_$T
head -n 12 $O/${T}_kernel_stats_16384_default_bench.csv | cut -c1-150
for W in d8 decay; do
  TDX_COMM_TRACE=1 timeout 600 python bench.py --gpus 8 --in-process --workload $W --steps 1 --warmup 1 --segments 2 --segments-out $O/${T}_segments_8strips_$W.json > $O/${T}_8strips_65536_$W.log 2> $O/${T}_8strips_65536_${W}_comm_trace.txt
  tail -n 1 $O/${T}_8strips_65536_$W.log > $O/${T}_8strips_65536_$W.json; rm -f $O/${T}_8strips_65536_$W.log
  python scripts/project_8gpu.py $O/${T}_segments_8strips_$W.json > $O/${T}_projection_8gpu_$W.txt; cat $O/${T}_projection_8gpu_$W.txt | cut -c1-160
  sort $O/${T}_8strips_65536_${W}_comm_trace.txt | uniq | grep taudem_amd > $O/${T}_tmp.txt; mv $O/${T}_tmp.txt $O/${T}_8strips_65536_${W}_comm_trace.txt
done
OUT_DIR=$O bash scripts/gpu_timeline.sh > /dev/null; cp $O/timeline/timeline.txt $O/${T}_timeline_d8_16384.txt
for m in "d8 16384" "d8 4096" "dinf 4096"; do set -- $m; taudem_amd/bin/tdxbench $1 -n $2 -steps 3 -crc 2>/dev/null | tail -n 1; done > $O/${T}_tdxbench_crc.jsonl
taudem_amd/bin/tdxbench decay -steps 1 -crc 2>/dev/null | tail -n 1 >> $O/${T}_tdxbench_crc.jsonl
cut -c1-300 $O/${T}_tdxbench_crc.jsonl
TDX_AD8_DEBUG=1 taudem_amd/bin/tdxbench d8 -n 16384 -steps 1 -warmup 0 2>&1 | grep "cycles per tile" > $O/${T}_ad8_tile_phases.txt
(cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof3_$T -o r -- $R/taudem_amd/bin/tdxbench dinf -n 32768 -steps 2 -warmup 1 > $O/${T}_tdxbench_dinf_32768.json 2> $O/prof3_$T.log)
find $O/prof3_$T -name "*kernel_stats.csv" | head -n 1 | xargs -I{} cp {} $O/${T}_kernel_stats_dinf_32768.csv
rm -rf $O/prof3_$T
cd /tmp
for pass in sq fetch write; do
  case $pass in fetch) C="FETCH_SIZE";; write) C="WRITE_SIZE";; sq) C="SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU";; esac
  timeout 300 rocprofv3 --pmc $C --output-format csv -d $O/pmc_$pass -o p -- python $R/bench.py --full --cpu-sample 0 --no-extras --steps 2 --warmup 1 > $O/pmc_$pass.log 2>&1
  python $R/scripts/pmc_summary.py $O/pmc_$pass $O/${T}_pmc_${pass}_summary.json | head -n 3
  rm -rf $O/pmc_$pass
done

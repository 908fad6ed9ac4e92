#!/bin/bash
# record run of a round (r05, r06, ...): full -m gpu suite, bench lines (the full run and a plain driver-style one), launch tables, written
# to <output dir>.  Usage: bash tools/record_run.sh <tag> <output dir>
TAG=${1:-r05}
O=${2:?usage: bash tools/record_run.sh <tag> <output dir>}
mkdir -p "$O"
timeout -k 10 900 python -m pytest tests -m gpu -q --timeout 600 > "$O/${TAG}_gpu_tests.log" 2>&1
rc=$?
tail -3 "$O/${TAG}_gpu_tests.log"
if [ $rc -gt 1 ]; then echo "pytest rc=$rc: stopping"; exit $rc; fi
cp gpurun_out/e2e_parity.json gpurun_out/${TAG}_e2e_parity.json 2>/dev/null
timeout -k 10 600 python bench.py --steps 20 --warmup 5 > "$O/${TAG}_bench_steps20_warmup5.json" 2> "$O/${TAG}_bench_steps20_warmup5.err" || exit 1
timeout -k 10 600 python bench.py --full > "$O/${TAG}_bench.json" 2> "$O/${TAG}_bench.err" || exit 1
grep -h "steps in" "$O/${TAG}_bench_steps20_warmup5.err" "$O/${TAG}_bench.err"
timeout -k 10 300 python tools/ab_launches.py 8 0 > "$O/${TAG}_launches_b8.txt" 2>&1 || exit 1
timeout -k 10 300 python tools/ab_launches.py 1 0 > "$O/${TAG}_launches_b1.txt" 2>&1 || exit 1
timeout -k 10 300 python tools/launch_table.py 8 1 > "$O/${TAG}_launch_table_b8_pair.txt" 2>&1 || exit 1
timeout -k 10 300 python tools/launch_table.py 1 1 > "$O/${TAG}_launch_table_b1_pair.txt" 2>&1 || exit 1
exit $rc

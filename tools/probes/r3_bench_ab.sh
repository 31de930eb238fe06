#!/bin/bash
# whole-step A/B of the two circuit kernels through bench.py (same box): options reg_wires = 4 / read_map = 0, then 3 / 1
cd "$(dirname "$0")/../.."
LOGS=${LOGS:-build/r3_bench}     # one log per run
mkdir -p "$LOGS"
for cfg in ${CFGS:-"4 0" "3 1"}; do
  set -- $cfg
  for wl in ${WLS:-n16_L6_dense n12_L4_dense n8_L4_dense}; do
    timeout -k 10 300 python bench.py --opt reg_wires=$1 --opt read_map=$2 --steps ${STEPS:-20} --warmup 5 --workload $wl --no-cpu-baseline --no-gate-bench --series none --no-extras > "$LOGS/$1_$2_$wl.log" 2>&1
    rc=$?
    tail -1 "$LOGS/$1_$2_$wl.log" | python -c "import json,sys; r=json.loads(sys.stdin.read()); print('reg_wires $1 read_map $2 $wl', 'steps/s', round(r['value'],2), 'ms', r['ms_per_step'], r.get('phase_ms'))" || tail -3 "$LOGS/$1_$2_$wl.log"
    if [ $rc -ge 124 ]; then echo "timed out"; exit 1; fi
  done
done

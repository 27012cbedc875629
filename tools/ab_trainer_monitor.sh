#!/bin/bash
# A/B of the harmonic cooling driver's Trainer loop (tools/bench_loop.py --physics ho --trainer K) without and with the
# episodes' performance and a train.Monitor (--monitor), alternating, two rounds each, at 65 536 envs ('xp', deferred
# reset); episodes are shortened to T_MAX time units so that every env finishes and the actor is pushed within the timed
# steps. Then, in a run of its own, the --monitor loop under rocprofv3 --kernel-trace --stats: the monitor's and the env
# tail kernel's own times, and the sum of all kernels' times against the loop's wall time. Results go to the directory
# given as the first argument (default: ab_trainer_out).
set -u -o pipefail
cd "$(dirname "$0")/.."
K="${K:-8}"; B="${B:-65536}"; STEPS="${STEPS:-45}"; T_MAX="${T_MAX:-0.5}"
OUT="${1:-ab_trainer_out}"
mkdir -p "$OUT"
for round in 1 2; do
  for mode in plain monitor; do
    flag=""; [ "$mode" = monitor ] && flag="--monitor"
    timeout -k 10 240 python tools/bench_loop.py --physics ho --batch "$B" --steps "$STEPS" --reset deferred --t-max "$T_MAX" \
      --trainer "$K" $flag > "$OUT/ab_trainer_monitor_${mode}_$round.json" 2> "$OUT/ab_trainer_monitor_${mode}_$round.err" || exit $?
    python3 -c "import json,sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print(sys.argv[2], sys.argv[3], '%.3f ms per control step' % d['ms_per_control_step'], d.get('monitor_receives', ''))" \
      "$OUT/ab_trainer_monitor_${mode}_$round.json" "$mode" "$round" || exit $?
  done
done
if command -v rocprofv3 > /dev/null; then
  PROF="$(mktemp -d)"
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$PROF" -- \
    python tools/bench_loop.py --physics ho --batch "$B" --steps "$STEPS" --reset deferred --t-max "$T_MAX" --trainer "$K" --monitor \
    > "$OUT/ab_trainer_monitor_prof.json" 2> "$OUT/ab_trainer_monitor_prof.err" || exit $?
  find "$PROF" -name '*kernel_stats.csv' -exec cp {} "$OUT/ab_trainer_monitor_kernel_stats.csv" \;
  grep -h "k_monitor_receive\|k_env_tail\|k_sched_tick" "$OUT/ab_trainer_monitor_kernel_stats.csv"
  python3 -c "import csv,sys; r=list(csv.DictReader(open(sys.argv[1]))); print('all kernels: %.3f ms in total' % (sum(float(x['TotalDurationNs']) for x in r) / 1e6))" \
    "$OUT/ab_trainer_monitor_kernel_stats.csv"
  rm -rf "$PROF"
fi

#!/bin/bash
# A/B of the hand-written loop (tools/bench_loop.py --reset deferred --learn K) against the same objects through
# train.Trainer.step (--trainer K), alternating, two rounds each, at 65 536 envs ('xp'); then, in a run of its own,
# the --trainer loop under rocprofv3 --kernel-trace --stats for the tick kernel's own time. Results go to the directory
# given as the first argument (default: ab_trainer_out).
set -u -o pipefail
cd "$(dirname "$0")/.."
K="${K:-8}"; B="${B:-65536}"; STEPS="${STEPS:-40}"
OUT="${1:-ab_trainer_out}"
mkdir -p "$OUT"
for round in 1 2; do
  for mode in learn trainer; do
    timeout -k 10 240 python tools/bench_loop.py --batch "$B" --steps "$STEPS" --reset deferred "--$mode" "$K" \
      > "$OUT/ab_trainer_${mode}_$round.json" 2> "$OUT/ab_trainer_${mode}_$round.err" || exit $?
    python3 -c "import json,sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print(sys.argv[2], sys.argv[3], '%.3f ms per control step' % d['ms_per_control_step'])" \
      "$OUT/ab_trainer_${mode}_$round.json" "$mode" "$round" || exit $?
  done
done
if command -v rocprofv3 > /dev/null; then
  rm -rf "$OUT/ab_trainer_prof"
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/ab_trainer_prof" -- \
    python tools/bench_loop.py --batch "$B" --steps "$STEPS" --reset deferred --trainer "$K" \
    > "$OUT/ab_trainer_prof.json" 2> "$OUT/ab_trainer_prof.err" || exit $?
  grep -rh "k_sched_tick" "$OUT/ab_trainer_prof" --include='*kernel_stats.csv' | head -3
fi

#!/bin/bash
# ms per step of the driver's bench command under rt_set_tuning knobs: tools/knob_sweep.sh "mask_identity=1" "mk_w_leaf=24" ...
cd "$GRAFT_REPO_ROOT" 2>/dev/null || cd "$(dirname "$0")/.."
tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
for t in "" "$@"; do
  timeout -k 10 300 python3 bench.py --full --steps 20 --warmup 5 --cpu-seconds 0 --no-in-flight-check --per-step-dispatches 0 ${t:+--tune $t} > $tmp/knob.json 2> $tmp/knob.err || { echo "$t failed"; tail -3 $tmp/knob.err; continue; }
  python3 -c "
import json,sys
d=json.loads([l for l in open('$tmp/knob.json') if l.startswith('{')][-1]); r=d['roofline']
print(f\"{'$t' or 'default':32s} {d['ms_per_step']:8.2f} ms/step  trace {r['avg_launch_ms']:.3f} ms x {r['launches']:.0f}\", flush=True)"
done

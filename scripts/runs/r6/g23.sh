#!/bin/bash
# Round 6, call g23: defaults re-checked after the round's byte cuts -- driver bench per setting, interleaved x2
set -o pipefail
O=gpurun_out/r6/g23
mkdir -p $O
run() {  # tag, env assignments...
  local t=$1; shift
  env "$@" timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 >> $O/$t.jsonl 2>> $O/err.log || { echo "$t failed"; tail $O/err.log; exit 1; }
}
for i in 1 2; do
  run base DLA_NOOP=1
  run defer_auto DLA_WGRAD_DEFER=auto
  run splitk768 DLA_SPLITK_BLOCKS=768
  run bnred2048 DLA_BN_RED_BLOCKS=2048
  run bnred512 DLA_BN_RED_BLOCKS=512
  run hiprio DLA_COMPUTE_STREAM=high
  echo "round $i done"
done
python3 - <<'PY'
import json, glob, os
for f in sorted(glob.glob("gpurun_out/r6/g23/*.jsonl")):
    v = [json.loads(l) for l in open(f) if l.startswith("{")]
    print(os.path.basename(f)[:-6], [round(d["value"]) for d in v], [d["ms_per_step"] for d in v],
          [d["telemetry"]["before_timed"]["gfxclk_mhz"] for d in v])
PY

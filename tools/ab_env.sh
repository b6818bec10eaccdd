#!/bin/bash
# On the GPU box: the bench line of the default library under two values of one environment switch, batched launch only.
#   tools/ab_env.sh SMAFA_ZONE_DIRECT "0 1" [bench flags]
cd "$(dirname "$0")/.."
export OUT=${OUT:-bench_out}
mkdir -p "$OUT"
var=$1; vals=$2; shift 2
for v in $vals; do
  env $var=$v python3 bench.py --full --no-cpu-baseline --no-stream --steps 30 "$@" > "$OUT/abenv.json" 2> "$OUT/abenv.err"
  python3 - "$var=$v" <<'PY'
import json, os, sys
d = json.load(open(os.environ["OUT"] + "/abenv.json"))
print("%-24s %.3f ms/launch  %.3f M q/s  verified=%s  %s" % (sys.argv[1], d["roofline"]["kernel_ms_avg"], d["value"] / 1e6, d["verified"], d["roofline"]["kernel"]))
PY
done

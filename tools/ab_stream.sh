#!/bin/bash
# One-query-per-pass figures of the default library and of every smafa_amd/lib_v*/ build (run on the GPU box).
cd "$(dirname "$0")/.."
export OUT=${OUT:-bench_out}
mkdir -p "$OUT"
run() {
  SMAFA_AMD_LIB=$2 python3 bench.py --full --no-cpu-baseline --no-related --steps 5 --full-record "$OUT/abs_$1_full.json" "${@:3}" > "$OUT/abs_$1.json" 2> "$OUT/abs_$1.err"
  python3 - "$1" <<'PY'
import json, os, sys
d = json.load(open(os.environ["OUT"] + "/abs_%s_full.json" % sys.argv[1])); s = d["stream"]["metric_store"]["shipped"]
print("%-8s one query: kernel %.1f us  wall %.1f us  %s  verified=%s" % (sys.argv[1], s["kernel_ms_median"] * 1e3, s["ms_per_query_wall"] * 1e3, s["kernel"], d["verified"]))
PY
}
run base "" "$@"
for lib in smafa_amd/lib_v*/libsmafa_amd.so; do
  [ -f "$lib" ] || continue
  run $(basename $(dirname $lib)) "$PWD/$lib" "$@"
done

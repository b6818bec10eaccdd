#!/bin/bash
# A/B of scan-kernel variants on the GPU box.  Run-time knobs (no rebuild): SMAFA_TILES=1|2 (wave tiles per
# wave), SMAFA_FILTER=0|1, SMAFA_NT_PLANES=3.  Build-time knobs go through EXTRA (e.g. -DSMAFA_ZONE_WAVES_10=4).
set -u
cd "$(dirname "$0")/.."
export OUT=${OUT:-bench_out}
mkdir -p "$OUT"
if [ -n "${EXTRA:-}" ]; then make -C smafa_amd/csrc -B -j8 EXTRA_HIPFLAGS="$EXTRA" > /dev/null 2>&1 || { echo "build failed"; exit 1; }; fi
for alpha in ${ALPHABETS:-aa nt}; do
  for tiles in ${TILES:-1 2}; do
    for rep in 1 2; do
      if [ "$alpha" = nt ]; then args="--alphabet nt --max-div 3 --queries 100000"; else args=""; fi
      SMAFA_TILES=$tiles timeout -k 10 150 python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --no-stream $args ${BENCH_ARGS:-} > "$OUT/var.json" 2> "$OUT/var.err"
      python - "$alpha" "$tiles" <<'PY'
import json, os, sys
try:
    d=json.load(open(os.environ["OUT"] + "/var.json"))
    print(f"{sys.argv[1]} tiles/wave={sys.argv[2]}  q/s={d['value']:.0f}  kernel_ms={d['roofline']['kernel_ms_avg']:.3f} verified={d['verified']} B/subject={d['roofline']['stored_bytes_per_subject']}")
except Exception as e:
    print(f"{sys.argv[1]} tiles={sys.argv[2]} FAILED {e}")
PY
    done
  done
done
if [ -n "${EXTRA:-}" ]; then make -C smafa_amd/csrc -B -j8 > /dev/null 2>&1; fi

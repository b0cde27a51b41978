#!/bin/bash
# End-of-round evidence on one MI355X, from the tree as committed: STEP=tests -- full `pytest -m gpu`, smoke(), the
# whole bench (`python bench.py --full --gpus 1 --steps 20 --warmup 5`); STEP=prof -- rocprofv3 kernel stats of
# the headline bench and of the whole bench, and the per-stage PMC passes (tools/pmc_all.sh) for MODELS.
# Outputs: $OUT/final_* (OUT defaults to check_out/ in the repository root).
# Each GPU step has its own time limit; the first failure ends the call.
cd "$(dirname "$0")/.." || exit 1; OUT=${OUT:-check_out}; mkdir -p "$OUT"; export TMPDIR=/tmp
if [ "${STEP:-tests}" = tests ]; then
  timeout -k 10 900 python -u -m pytest tests -m gpu -q --timeout 300 --timeout-method thread > "$OUT/final_gputests.log" 2>&1 || { tail -30 "$OUT/final_gputests.log"; exit 1; }
  tail -1 "$OUT/final_gputests.log"
  timeout -k 10 150 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/final_smoke.log" 2>&1 || { tail -20 "$OUT/final_smoke.log"; exit 1; }
  tail -2 "$OUT/final_smoke.log"
  timeout -k 10 400 python bench.py --full --gpus 1 --steps 20 --warmup 5 > "$OUT/final_bench.json" 2> "$OUT/final_bench.err" || { tail -20 "$OUT/final_bench.err"; exit 1; }
  tail -1 "$OUT/final_bench.json" | cut -c1-600
else
  rm -rf "$OUT/final_prof" "$OUT/final_prof_all"
  # the headline alone (its kernels' averages are the bench line's per-launch figures), then the whole --full
  # bench (the NAS / config-5 / train / eval512 legs' kernels; k_c12s there also averages the small batches)
  timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$OUT/final_prof" -o run --output-format csv -- python bench.py --steps 20 --warmup 5 > "$OUT/final_prof.log" 2>&1 || { tail -20 "$OUT/final_prof.log"; exit 1; }
  python tools/top_kernels.py "$(find "$OUT/final_prof" -name '*kernel_stats.csv' | head -1)"
  timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$OUT/final_prof_all" -o run --output-format csv -- python bench.py --full --no-cpu-baseline --steps 20 --warmup 5 > "$OUT/final_prof_all.log" 2>&1 || { tail -20 "$OUT/final_prof_all.log"; exit 1; }
  MODELS="${MODELS:-hardnet wang2 wang3 wang4 c5}" timeout -k 10 900 bash tools/pmc_all.sh || exit 1
fi
echo done

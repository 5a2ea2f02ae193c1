#!/bin/bash
# The end-of-work check on a GPU box, from anywhere inside the checkout:  bash tools/gpu_full_check.sh [OUTDIR]
# `pytest -m gpu`, the full benchmark line (`bench.py --full`) with a summary of every record, `smoke()`.  Logs go to OUTDIR (default: a new
# temporary directory, printed); the first step that fails ends the script with its exit status.
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
OUT=${1:-$(mktemp -d)}
mkdir -p "$OUT" && echo "logs in $OUT"
export TMPDIR=/tmp
timeout -k 10 2700 python -m pytest tests -q -m gpu > "$OUT/gputests.log" 2>&1; rc=$?
echo "gpu rc=$rc"; tail -6 "$OUT/gputests.log"; [ $rc = 0 ] || exit $rc
timeout -k 10 900 python bench.py --full > "$OUT/bench_full.log" 2> "$OUT/bench_full.err"; rc=$?
echo "bench rc=$rc"; tail -3 "$OUT/bench_full.err"; [ $rc = 0 ] || exit $rc
python - "$OUT/bench_full.log" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
c = d["config"]
print("headline", d["value"], d["ms_per_step"], c["ms_per_step_one_batch_in_flight"], c["pairs_per_s_with_host_ids_h2d"],
      c["h2d_inclusive_over_resident_sustained"], c["macro_batch"])
print({k: v for k, v in d["roofline"].items() if k != "kernels_us_per_step"})
for e in d["sub"]:
    print(e["name"], e.get("pairs_per_s"), e.get("ms_per_step"), e.get("frac"), e.get("bound"), e.get("error"))
PY
timeout -k 10 600 python __graft_entry__.py --smoke 2>&1 | tail -6

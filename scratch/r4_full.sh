#!/bin/bash
# full gpu suite + the bench line; usage: r4_full.sh OUT_DIR
cd "$(dirname "$0")/.."; O=${1:?usage: r4_full.sh OUT_DIR}; mkdir -p "$O"
timeout 900 python -m pytest tests -x -q -m gpu > $O/r4_gpu_tests.log 2>&1; tail -4 $O/r4_gpu_tests.log
timeout 600 python bench.py --full > $O/r4_bench.json 2> $O/r4_bench.err; python - "$O/r4_bench.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().split("\n")[-1])
print("ms_per_step", d["ms_per_step"], "value", d["value"], "step_frac", d["roofline"].get("step_frac"))
for k,v in d.get("roofline_all",{}).items(): print("  %-24s %8.1f us  frac %.3f  us/step %s" % (k, v["avg_launch_us"], v["frac"], v.get("us_per_step")))
PY

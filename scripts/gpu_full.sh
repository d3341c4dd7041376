#!/bin/bash
# whole GPU suite + smoke() + the default line with everything `bench.py --full` adds, at HEAD; results under $OUT_DIR (default results/)
cd $GRAFT_REPO_ROOT
export OUT=${OUT_DIR:-results}
mkdir -p $OUT
timeout 2400 python -m pytest tests -m gpu -x -q --durations=8 2>&1 | tail -25 > $OUT/full_pytest.log
tail -22 $OUT/full_pytest.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -3
timeout 900 python bench.py --steps 20 --warmup 3 --full > $OUT/bench20.json 2> $OUT/bench20.err; echo "bench rc=$?"
python - <<'PY'
import json, os
d = json.load(open(os.path.join(os.environ["OUT"], "bench20.json")))
print({k: d[k] for k in ("value", "ms_per_step")}, d["roofline"]["frac"], d["cpu_baseline"]["value"])
print({k: (v.get("value"), v.get("error")) for k, v in d["extra"].items()})
print(d["extra"]["fine_tune"].get("roofline", {}).get("frac"), d["extra"]["mattergen_shaped_sampler"].get("hbm_roofline"))
PY
tail -3 $OUT/bench20.err

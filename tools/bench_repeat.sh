#!/bin/bash
# tools/bench_repeat.sh [N] [OUTDIR] -- on the GPU box: the driver's command with every configuration measured
# (`python3 bench.py --gpus 1 --steps 20 --warmup 5 --full`) in N fresh processes, one after the other; every line goes to
# OUTDIR/bench_repeat.jsonl and a min / median / max table of every configuration's roofline fraction and ms_per_step to
# OUTDIR/bench_repeat_summary.json (OUTDIR: bench_repeat_out)
N=${1:-5}
OUT=${2:-bench_repeat_out}
mkdir -p "$OUT"
: > "$OUT/bench_repeat.jsonl"
for i in $(seq 1 $N); do
  timeout -k 10 900 python3 bench.py --gpus 1 --steps 20 --warmup 5 --full >> "$OUT/bench_repeat.jsonl" 2>> "$OUT/bench_repeat.err" || exit 1
  echo "run $i done"
done
OUT="$OUT" python3 - <<'PY'
import json, os, statistics
out_dir = os.environ["OUT"]
lines = [json.loads(l) for l in open(os.path.join(out_dir, "bench_repeat.jsonl")) if l.startswith("{")]
def col(get):
    v = sorted(get(l) for l in lines)
    return {"min": v[0], "median": statistics.median(v), "max": v[-1], "all": v}
out = {"runs": len(lines), "command": "python3 bench.py --gpus 1 --steps 20 --warmup 5 --full (fresh process each)",
       "c2": {"frac": col(lambda l: l["roofline"]["frac"]), "ms_per_step": col(lambda l: l["ms_per_step"])}}
for k in ("c3", "c4", "c2_values"):
    out[k] = {"frac": col(lambda l: l["secondary"][k]["roofline"]["frac"]), "ms_per_step": col(lambda l: l["secondary"][k]["ms_per_step"])}
nr = [l["secondary"]["next_rows"] for l in lines if "materialize" in l["secondary"].get("next_rows", {})]
if nr:
    out["materialize_ms"] = sorted(x["materialize"]["ms"]["median"] for x in nr)
    out["permutation_ms"] = sorted(x["permutation"]["ms"]["median"] for x in nr)
json.dump(out, open(os.path.join(out_dir, "bench_repeat_summary.json"), "w"), indent=1)
print(json.dumps({k: (v["frac"] if isinstance(v, dict) and "frac" in v else v) for k, v in out.items()}, indent=1))
PY

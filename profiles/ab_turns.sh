#!/bin/bash
# Two builds of libvdjx.so in turns through VDJX_LIB_PATH, one bench.py line per run (profiles/r08_part_records.md):
#   profiles/ab_turns.sh OUTDIR RUNS PARENT.so CHANGE.so [bench.py arguments, e.g. --k 25 --mf 2 --mq 60 --mrs 20]
# prints "<library> <run> <ms per step>" per run and mean / sd per library at the end; every run under its own time limit, the first
# that fails ends the script.
set -o pipefail
out=$1; runs=$2; parent=$(readlink -f "$3"); change=$(readlink -f "$4"); shift 4
cd "$(dirname "$0")/.." || exit 1
mkdir -p "$out"
for i in $(seq 1 "$runs"); do
  for side in parent change; do
    so=$parent; [ $side = change ] && so=$change
    VDJX_LIB_PATH=$so timeout -k 10 300 python bench.py --gpus 1 --no-cpu "$@" > "$out/${side}_$i.json" 2> "$out/${side}_$i.err" || exit $?
    python -c "import json,sys; print('$side', $i, json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])['ms_per_step'])" "$out/${side}_$i.json"
  done
done
python - "$out" "$runs" <<'PY'
import json, statistics as st, sys
out, runs = sys.argv[1], int(sys.argv[2])
for side in ("parent", "change"):
    v = [json.loads(open(f"{out}/{side}_{i}.json").read().strip().splitlines()[-1])["ms_per_step"] for i in range(1, runs + 1)]
    print(side, v, "mean %.3f sd %.3f" % (st.mean(v), st.stdev(v) if len(v) > 1 else 0.0))
PY

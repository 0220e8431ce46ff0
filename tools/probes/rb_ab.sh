# A/B runs of bench.py on one box: bash tools/probes/rb_ab.sh "name ENV=.. ENV=.." ...   (one quoted argument per configuration)
O=${O:-$(mktemp -d)}; mkdir -p $O; echo "records: $O"
for cfg in "$@"; do
  set -- $cfg
  name=$1; shift
  env "$@" python bench.py --full --no-cpu-baseline --no-student --steps 10 > $O/ab_$name.json 2>$O/ab_$name.err
  python - <<PY
import json
d=json.load(open("$O/ab_$name.json"))
print("$name", d["value"], d["ms_per_step"], "sum of kernels", round(sum(k["ms_per_update"] for k in d["kernels"]), 3))
for k in d["kernels"][:9]: print("   ", k["name"][:60], k["launches_per_update"], k["avg_us"], k["ms_per_update"])
for l in d["roofline"]["levels"]: print("   L", l["level"][:50], l["avg_us"], l["frac"])
PY
done

export OUT=${OUT:-bench_out}
mkdir -p "$OUT"
for i in 1 2; do
  for v in "CSSM_WAVE_SUMS=0" "CSSM_WAVE_SUMS=1" "CSSM_WAVE_SUMS=1 CSSM_NO_OFFW=1"; do
    env $v python3 bench.py --steps 20 --warmup 5 --full --no-cpu --no-pmc --no-generic > "$OUT"/abq.json 2>/dev/null || exit 1
    python3 - "$v" <<'PY'
import json, os, sys
j = json.loads(open(os.path.join(os.environ["OUT"], "abq.json")).read().strip().splitlines()[-1]); r = j["roofline_16m"]
print(sys.argv[1], "2^24 d3:", {k: round(v, 1) for k, v in r["c2_d3"]["kernels_us"].items()}, "d1:", {k: round(v, 1) for k, v in r["c1_d1"]["kernels_us"].items()})
PY
  done
done

OUT=${1:?usage: tools/overlap_check.sh <outdir>}
mkdir -p $OUT; rm -f $OUT/*.json
python -m pytest tests/test_gpu_torch_side.py tests/test_gpu_bench.py -m gpu -q -x > $OUT/t.log 2>&1; echo rc=$? >> $OUT/t.log; tail -n 15 $OUT/t.log
for f in "" "--overlap-gather"; do
  python bench.py --full --force-comm --graph on $f --no-c5 --no-cpu-baseline --envs 8192 --steps 960 --warmup 96 > $OUT/graph_8k$f.json 2>/dev/null
  python bench.py --full --force-comm --graph on $f --no-c5 --no-cpu-baseline --steps 960 --warmup 96 > $OUT/graph_64k$f.json 2>/dev/null
  python bench.py --full --force-comm --graph off $f --no-c5 --no-cpu-baseline --envs 8192 --steps 960 --warmup 96 > $OUT/eager_8k$f.json 2>/dev/null
done
python - $OUT <<PY
import json,glob,sys
for f in sorted(glob.glob(sys.argv[1] + "/*.json")):
    t=open(f).read().strip().splitlines()
    if not t: print(f, "EMPTY"); continue
    d=json.loads(t[-1]); p=d["phases"]
    print(f, "ms/step %.4f"%d["ms_per_step"], "expected %.4f"%p["expected_ms_per_step"], p["expected_bound"], {k: round(v,2) for k,v in p["per_rank"][0].items()})
PY

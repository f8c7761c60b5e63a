cd "$GRAFT_REPO_ROOT" || exit 1
O=${OUT:?set OUT to the folder the result lines go to}
mkdir -p "$O"
for r in 1 2; do
  for b in 2 3 4 1; do
    PMC_FRONT_BATCH=$b timeout -k 10 300 python bench.py --full --no-cpu-baseline > "$O/b${b}_$r.json" 2> "$O/b${b}_$r.err" || exit $?
    python3 -c "import json; d=json.load(open('$O/b${b}_$r.json')); print('batch $b run $r', round(d['value'],3), round(d['roofline']['kernel_ms_per_step']['pmc::deflate_front_kernel'],1))"
  done
done

# A/B of library variants / environment switches on one box:  bash tools/ab.sh "ENV=1" "ENV=0" ...   (kernel tuning only)
for i in 1 2; do for v in "$@"; do env $v python bench.py --full --steps 200 --warmup 20 --no-cpu-baseline | python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$v', d['ms_per_step'], d['ms_per_step_stats']['median'], d['roofline']['kernel_ms_avg'], d['with_cached_weight_operands']['ms_per_step'])
"; done; done

# A/B of one environment variable on one box: tools/ab_env.sh VAR v1 v2 ...
o=${BENCH_AB_OUT:-$(mktemp -d)}     # where the bench lines of the runs go (default: a fresh temporary directory)
var=$1; shift
i=0
for v in "$@"; do
i=$((i+1))
env $var=$v python bench.py --full --no-cpu-baseline --no-overlap-probe --no-solo-probe --no-extra-workloads > $o/b_$i.json 2> $o/b_$i.err && python -c "
import json,sys; d=json.load(open('$o/b_$i.json')); print('$var=$v', round(d['value'],1), d['ms_per_step'], d['kernel_ms']['ransac_pre'], d['kernel_ms']['ransac_eval'], d['kernel_ms']['ransac_hyp'], d['ransac_prefilter']['survivors'], d['roofline']['avg_launch_ms'])" || exit 1
done

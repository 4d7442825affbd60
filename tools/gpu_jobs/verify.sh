#!/bin/bash
# Re-verifies a build on the GPU box and collects the evidence committed under profiles/:
#   bash tools/gpu_jobs/verify.sh <tag> [output folder, default /tmp/pfa_verify_<tag>]
# GPU test suite, smoke(), the full bench line (--full: with self_check and cpu_baseline), a sustained run (1500 steps) and the
# rocprofv3 kernel statistics of the full bench command.  Outputs: <output folder>/<tag>_* (bench lines, their stderr, logs, statistics).
TAG=${1:-verify}
OUT=${2:-/tmp/pfa_verify_$TAG}
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd) || exit 1
ROOT=$PWD
timeout 400 python -m pytest tests -m gpu -x -q > $OUT/${TAG}_tests.log 2>&1; echo "tests rc=$?"
grep -n "passed\|failed" $OUT/${TAG}_tests.log | tail -3
timeout 200 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1; echo "smoke rc=$?"
timeout 300 python bench.py --full > $OUT/${TAG}_bench_mlp.json 2> $OUT/${TAG}_bench_mlp.err; echo "bench rc=$?"
timeout 100 python bench.py --full --steps 1500 --warmup 20 --no-cpu-baseline --no-breakdown > $OUT/${TAG}_bench_mlp_sustained.json 2> $OUT/${TAG}_bench_mlp_sustained.err; echo "sustained rc=$?"
( cd /tmp && export TMPDIR=/tmp && timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_ks_mlp -o ks -- python $ROOT/bench.py --full --steps 10 --no-cpu-baseline --no-breakdown > $OUT/${TAG}_ks_mlp.log 2>&1; echo "rocprof rc=$?" )
find $OUT/${TAG}_ks_mlp -name "*kernel_stats.csv" -exec cp {} $OUT/${TAG}_kernel_stats_mlp.csv \;
rm -rf $OUT/${TAG}_ks_mlp
python - "$OUT" "$TAG" <<'PY'
import json, os, sys
out, tag = sys.argv[1:]
for n in ('bench_mlp', 'bench_mlp_sustained'):
    lines = [ln for ln in open(os.path.join(out, f'{tag}_{n}.json')) if ln.startswith('{')]
    if not lines:
        print(n, 'printed no result line; the end of its stderr:')
        print(open(os.path.join(out, f'{tag}_{n}.err')).read()[-3000:])
        continue
    d = json.loads(lines[-1])
    print(n, round(d['value'] / 1e6, 1), 'M steps/s', round(d['ms_per_step'], 4), 'ms', 'grad', round(d['roofline']['avg_launch_ms'] * 1e3, 2), 'us frac',
          round(d['roofline']['frac'], 3), d.get('self_check', {}).get('max_abs_weight_err'), d.get('cpu_baseline', {}).get('value'))
PY
head -6 $OUT/${TAG}_kernel_stats_mlp.csv | cut -c1-160

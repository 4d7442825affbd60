#!/bin/bash
# c3 (LSTM 128 on 160-float rows, 4096 envs): bench line + per-kernel event breakdown
timeout 500 python bench.py --full --workload c3 --steps 5 --warmup 2 --no-cpu-baseline --no-extra --sustained-seconds 0 2>/dev/null | python -c "
import json, sys
d = json.loads([l for l in sys.stdin.read().splitlines() if l.startswith('{')][0])
print('value', d['value'], 'ms', d['ms_per_step'])
for k in d:
    if 'break' in k or 'kernel' in k:
        print(k, json.dumps(d[k])[:2500])"

#!/bin/bash
# Same-box A/B of the block-buffer row alignment, regression step, alternating, two repetitions:
#   EML_ROW_ALIGN=16/32  block-buffer rows of whole 128-byte lines (block 2: 304 -> 320 floats)
REPO=${GRAFT_REPO_ROOT:-/root/repo}
cd /tmp && export TMPDIR=/tmp
for rep in 1 2; do
for align in 16 32; do
  ( export EML_ROW_ALIGN=$align
  timeout 300 python $REPO/bench.py --steps 10 --warmup 3 --no_cpu_baseline --legs families 2>/dev/null | python -c "
import json,sys
j=json.loads(sys.stdin.read().strip().splitlines()[-1])
f={r['kernel'][:22]: r['ms_per_step'] for r in j.get('kernel_families', [])}
print('align=$align %7.2f img/s %8.3f ms | %s' % (j['value'], j['ms_per_step'], {k: v for k, v in f.items() if v}))" )
done
done

#!/bin/bash
# A/B timing of library builds inside ONE GPU session (box-to-box variance is larger than most kernel changes):
#   bash tools/ab.sh 3 "" experiments/libA.so experiments/libB.so
# usage: tools/ab.sh ROUNDS "extra bench.py args" lib1.so lib2.so ...   (libs are alternated ROUNDS times)
# Each line: library, ms/step, sort_tiles + render_forward (the only figure of those two stages that compares across the
# commit that moved the short-list sort into the forward blend), per-stage ms (HIP events inside the library, see bench.py),
# then ms/step of the other_workloads.  Every run has a time limit of its own (AB_TIMEOUT seconds, default 600); the first
# run that fails or runs out of time ends the script with its status: nothing else is started on the GPU after it.
set -o pipefail
R=$1; shift; ARGS=$1; shift
for i in $(seq "$R"); do
  for L in "$@"; do
    SPLATRASTER_LIB=$(realpath "$L") timeout -k 10 "${AB_TIMEOUT:-600}" python bench.py --full --cpu-baseline none --steps 30 $ARGS | python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1]); s=d['stage_ms']
print('%-28s'%'$L', '%.4f'%d['ms_per_step'], 'sort+fwd=%.4f'%(s['sort_tiles']+s['render_forward']), ' '.join('%s=%.4f'%(k[:14],v) for k,v in s.items()),
      ' '.join('[%s: %.4f sort+fwd=%.4f]'%(w.get('name'), w['ms_per_step'], w['stage_ms']['sort_tiles']+w['stage_ms']['render_forward'])
               for w in d.get('other_workloads') or [] if 'stage_ms' in w and 'ms_per_step' in w))" || exit $?
  done
done

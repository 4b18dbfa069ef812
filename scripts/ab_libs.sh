#!/bin/bash
# A/B of library builds (POM_LIB): usage [REPS=3] [SHAPES="driver long ..."] ab_libs.sh lib1 lib2 ... ; the builds alternate within every
# repetition.  Shapes: driver (20 steps), long (500 steps: the default `python bench.py`), plain launch, stress, simple, tape, 262144 envs
# Every bench run has its own time limit (STEP_LIMIT seconds, default 300); the first run that fails or is cut off ends the script.
set -o pipefail
run() {
  timeout -k 10 ${STEP_LIMIT:-300} python3 bench.py --no-cpu-baseline --no-config3 "$@" 2>/dev/null | python3 -c "import sys,json; r=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('%.2f us %.2f G' % (r['ms_per_step']*1e3, r['value']/1e9))" \
    || { echo "bench.py $* failed (status ${PIPESTATUS[0]}): stopping"; exit 1; }
}
SHAPES=${SHAPES:-driver long plain stress simple tape big}
for rep in $(seq 1 ${REPS:-3}); do for lib in "$@"; do
  export POM_LIB=$PWD/$lib
  for shape in $SHAPES; do case $shape in
    driver) echo -n "$lib rep $rep  driver shape: "; run --steps 20 --warmup 5 ;;
    long)   echo -n "$lib rep $rep  500 steps: "; run --steps 500 --warmup 50 ;;
    plain)  echo -n "$lib rep $rep  plain launch: "; run --steps 200 --warmup 20 --streams 1 ;;
    stress) echo -n "$lib rep $rep  stress: "; run --steps 100 --warmup 20 --kind stress --dist stress ;;
    simple) echo -n "$lib rep $rep  simple: "; run --steps 100 --warmup 20 --policy simple ;;
    tape)   echo -n "$lib rep $rep  tape: "; run --steps 200 --warmup 20 --policy tape ;;
    big)    echo -n "$lib rep $rep  262144 envs: "; run --steps 100 --warmup 20 --envs 262144 ;;
  esac; done
done; done

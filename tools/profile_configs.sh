#!/bin/bash
# Every BASELINE configuration through bench.py: the JSON line of `bench.py --full --config c` (pipelined,
# sequential, sustained and exact-fp32 rates, kernels / convs tables, roofline, cpu_baseline) and a rocprofv3 kernel trace of
# the same workload with one batch in flight (per-step breakdown by launch grid).  Run on the GPU box; output under $OUT
# (default runs/); condense with `python tools/make_configs_profile.py r03 $OUT`.
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${OUT:-runs}
mkdir -p $OUT/configs
for c in ${CONFIGS:-1 2 3 4}; do
  python3 bench.py --full --config $c --steps 20 --warmup 3 --cpu-budget 25 > $OUT/configs/cfg$c.json 2> $OUT/configs/cfg$c.log || { tail -5 $OUT/configs/cfg$c.log; exit 1; }
  rm -rf $OUT/prof_cfg$c && mkdir -p $OUT/prof_cfg$c
  rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_cfg$c/kt -- python3 bench.py --config $c --no-cpu-baseline --no-extras --inflight 1 --steps 3 --warmup 2 > $OUT/prof_cfg$c/kt.log 2>&1 || { tail -5 $OUT/prof_cfg$c/kt.log; exit 1; }
  echo "config $c done: $(cut -c1-160 $OUT/configs/cfg$c.json)"
done

#!/bin/bash
# end-of-round evidence: GPU tests, the --full bench line, rocprofv3 kernel stats of the same command, PMC traffic
# usage: dev/round_profile.sh <tag>      e.g. r02_a   -> $OUT/<tag>_*, OUT defaults to out/  (copy what is to be judged into profiles/)
T=${1:-r02_x}
R=$PWD; export OUT=${OUT:-$R/out}; mkdir -p $OUT; rm -rf $OUT/${T}_prof $OUT/traffic_FETCH_SIZE $OUT/traffic_WRITE_SIZE
python -m pytest tests -q -m gpu 2>&1 | tail -2 | tee $OUT/${T}_gpu_tests.txt
python bench.py --full > $OUT/${T}_bench_neuralcf.json 2>$OUT/${T}_bench.err; tail -c 1500 $OUT/${T}_bench_neuralcf.json
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${T}_prof -- python3 $R/bench.py --full --no-cpu-baseline > $OUT/${T}_bench_under_rocprof.json 2>$OUT/${T}_prof.err
cd $R
cp $OUT/${T}_prof/*/*kernel_stats.csv $OUT/${T}_neuralcf_kernel_stats.csv
head -14 $OUT/${T}_neuralcf_kernel_stats.csv | cut -c1-150
bash dev/pmc_traffic.sh ${T}_neuralcf --steps 10 --warmup 3

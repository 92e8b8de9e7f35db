#!/bin/bash
# Round-end measurement recipe, run from the repo root on the GPU machine: bash scratch/run_round_profiles.sh OUTPUT_DIR
# (bench.py --full: the per-kernel timing loops and side measurements are part of what the traces and counters account for).
set -x
R=$PWD
O=$(realpath -m "${1:?usage: run_round_profiles.sh OUTPUT_DIR}")
mkdir -p $O
python bench.py --full > $O/bench_default.json 2> $O/bench_default.err
tail -c 3000 $O/bench_default.json
export TMPDIR=/tmp
cd /tmp
timeout 600 rocprofv3 --kernel-trace --stats -d $O/prof4s -o r -- python $R/bench.py --full --no-cpu-baseline --no-cobatch-extra > $O/prof4s.log 2>&1
timeout 600 rocprofv3 --kernel-trace --stats -d $O/prof1s -o r -- python $R/bench.py --full --no-cpu-baseline --no-cobatch-extra --streams 1 > $O/prof1s.log 2>&1
timeout 600 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/pmc_fetch -o r -- python $R/bench.py --full --no-cpu-baseline --no-cobatch-extra --streams 1 --steps 20 --warmup 5 > $O/pmc_fetch.log 2>&1
timeout 600 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/pmc_write -o r -- python $R/bench.py --full --no-cpu-baseline --no-cobatch-extra --streams 1 --steps 20 --warmup 5 > $O/pmc_write.log 2>&1
cd $R
ls -la $O $O/*
du -sh $O

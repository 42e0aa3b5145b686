#!/bin/bash
# The round's closing measurements on one box: profiles (tools/collect_profiles.sh), the full bench command, the per-layer table.
# usage (repo root): tools/exp/round_end.sh <tag> <output dir>
R=${GRAFT_REPO_ROOT:-$(pwd)}
TAG=${1:-rXX}
OUT=${2:?usage: tools/exp/round_end.sh <tag> <output dir>}
cd $R
mkdir -p $OUT
tools/collect_profiles.sh $TAG > $OUT/${TAG}_collect.log 2>&1
cd $R
timeout -s KILL 900 python bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/${TAG}_bench_default.log 2>&1
tail -1 $OUT/${TAG}_bench_default.log > $OUT/${TAG}_bench_default.json
timeout -s KILL 300 python bench.py --steps 3 --warmup 2 --no-cpu-baseline --no-extra --serial --per-layer > $OUT/${TAG}_per_layer.txt 2>&1
tail -3 $OUT/${TAG}_collect.log | cut -c1-300
cut -c1-600 $OUT/${TAG}_bench_default.json

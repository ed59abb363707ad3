#!/bin/bash
# Run on the GPU box: kernel-trace stats of the full bench + the two PMC passes that feed roofline.traffic.
# Usage: bash tools/profile_round.sh <tag> [batch]      -> $OUT/prof/<tag>_*  $OUT/pmc/<tag>_*   (OUT defaults to profile_out/)
set -e
TAG=${1:-r01}; B=${2:-512}
cd "$(dirname "$0")/.."; export TMPDIR=/tmp
OUT=${OUT:-profile_out}
mkdir -p $OUT/prof $OUT/pmc
rocprofv3 --kernel-trace --stats -d $OUT/prof -o ${TAG}_train --output-format csv -- python3 bench.py --full --batch $B --steps 5 --warmup 2 --no-decode --no-cpu-baseline > $OUT/prof_${TAG}_train.log 2>&1
rocprofv3 --kernel-trace --stats -d $OUT/prof -o ${TAG}_full --output-format csv -- python3 bench.py --full --batch $B --steps 5 --warmup 2 --no-cpu-baseline > $OUT/prof_${TAG}_full.log 2>&1
for C in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --kernel-trace --pmc $C -d $OUT/pmc -o ${TAG}_$C --output-format csv -- python3 bench.py --batch $B --steps 2 --warmup 1 > $OUT/pmc_${TAG}_$C.log 2>&1
done
python3 tools/pmc_traffic.py $OUT/pmc/${TAG}_FETCH_SIZE_counter_collection.csv $OUT/pmc/${TAG}_WRITE_SIZE_counter_collection.csv $OUT/pmc_traffic_b$B.json > $OUT/pmc_${TAG}_summary.txt
cat $OUT/pmc_${TAG}_summary.txt
grep metric $OUT/prof_${TAG}_train.log | cut -c1-200

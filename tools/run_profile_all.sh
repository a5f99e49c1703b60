# refresh everything under profiles/ from one box: tests, PMC traffic (two passes), the bench line, rocprofv3 stats
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
OUT=${1:-profile_out}            # output directory (first argument)
mkdir -p $OUT
timeout 900 python -m pytest tests -q -m gpu -x 2>&1 | tail -2
timeout 900 python tools/pmc_traffic.py 2>&1 | tail -3
cp profiles/pmc_traffic.json $OUT/pmc_traffic.json
python bench.py --full 2>&1 | tail -1 > $OUT/bench_default.json
cut -c1-900 $OUT/bench_default.json
rm -rf $OUT/prof_default
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_default -- python3 bench.py --full --no-cpu-baseline --no-also > $OUT/prof_default.log 2>&1
find $OUT/prof_default -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $OUT/kernel_stats_default.csv
rm -rf $OUT/prof_single
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_single -- python3 bench.py --steps 5 --warmup 2 --no-cpu-baseline --no-kernel-events --no-side-stream > $OUT/prof_single.log 2>&1
find $OUT/prof_single -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $OUT/kernel_stats_single.csv
find $OUT/prof_default $OUT/prof_single -type f -delete 2>/dev/null
head -8 $OUT/kernel_stats_default.csv | cut -c1-150

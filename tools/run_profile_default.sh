cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
OUT=${1:-profile_out}            # output directory (first argument)
mkdir -p $OUT
timeout 900 python -m pytest tests -q -m gpu -x 2>&1 | tail -3
python bench.py --full 2>&1 | tail -1 > $OUT/bench_default.json
cat $OUT/bench_default.json | cut -c1-1200
rm -rf $OUT/prof_default
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_default -- python3 bench.py --full --no-cpu-baseline --no-also > $OUT/prof_default.log 2>&1
tail -1 $OUT/prof_default.log | cut -c1-300
find $OUT/prof_default -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $OUT/kernel_stats_default.csv
head -12 $OUT/kernel_stats_default.csv | cut -c1-160
find $OUT/prof_default -type f ! -name "*kernel_stats.csv" -delete

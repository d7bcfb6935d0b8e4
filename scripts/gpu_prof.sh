# bench.py --full (no CPU baseline) + rocprofv3 kernel trace of a short bench run -> $OUT/prof (OUT: results
# directory, default out/ in the repository)
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}
cd $R && mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $OUT/bench.log 2>&1; rc=$?; echo "bench rc=$rc"
[ $rc -eq 0 ] || exit $rc
cd /tmp
rm -rf $OUT/prof
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof -o run --output-format csv -- python3 $R/bench.py --steps 10 --warmup 3 --full --no-cpu-baseline --no-roofline > $OUT/prof.log 2>&1; rc=$?; echo "prof rc=$rc"

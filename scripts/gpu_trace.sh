# rocprofv3 kernel trace of a short bench run (--full: the extras' kernels included) -> $OUT/prof_$1; critical-path
# summary (OUT: results directory, default out/ in the repository)
set -u
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/out}
cd $R && mkdir -p $OUT
export TMPDIR=/tmp
tag=${1:-cur}; shift || true
cd /tmp
rm -rf $OUT/prof_$tag
env "$@" timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof_$tag -o run --output-format csv -- python3 $R/bench.py --steps 10 --warmup 3 --full --no-cpu-baseline --no-roofline > $OUT/prof_$tag.log 2>&1; rc=$?; echo "prof rc=$rc"
[ $rc -eq 0 ] || exit $rc
cd $R
f=$(find $OUT/prof_$tag -name "*kernel_trace.csv" | head -1)
python scripts/step_critical.py $f 2 > $OUT/crit_$tag.txt; cat $OUT/crit_$tag.txt

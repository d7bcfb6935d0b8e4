# One GPU call: GPU test suite, smoke, bench (N=1, --full: headline + roofline + extras + CPU baseline), rocprofv3
# kernel-trace of the bench command, PMC passes (FETCH_SIZE; WRITE_SIZE; MFMA busy — each its own run)
# -> $OUT/pmc_traffic.json (OUT: results directory, default out/ in the repository).  Stops at the first failure.
# SKIP_TESTS=1 skips the test suite.
set -u
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R
OUT=${OUT:-$R/out}
mkdir -p $OUT
export TMPDIR=/tmp
if [ "${SKIP_TESTS:-0}" != "1" ]; then
  timeout -k 10 1200 python -u -m pytest tests -m gpu -x -q -rf --timeout 300 --timeout-method thread > $OUT/tests.log 2>&1; rc=$?; echo "tests rc=$rc"; tail -4 $OUT/tests.log
  [ $rc -eq 0 ] || exit $rc
  timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; rc=$?; echo "smoke rc=$rc"; tail -2 $OUT/smoke.log
  [ $rc -eq 0 ] || exit $rc
fi
timeout -k 10 600 python bench.py --full > $OUT/bench.log 2>&1; rc=$?; echo "bench rc=$rc"; tail -c 1500 $OUT/bench.log
[ $rc -eq 0 ] || exit $rc
BENCH="python3 $R/bench.py --steps 10 --warmup 3 --full --no-cpu-baseline --no-extras"
cd /tmp
rm -rf $OUT/prof $OUT/pmc_fetch $OUT/pmc_write $OUT/pmc_mfma
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof -o run --output-format csv -- $BENCH > $OUT/prof.log 2>&1; rc=$?; echo "prof rc=$rc"
[ $rc -eq 0 ] || exit $rc
timeout -s KILL 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/pmc_fetch -o run --output-format csv -- $BENCH --no-roofline > $OUT/pmc_fetch.log 2>&1; rc=$?; echo "pmc fetch rc=$rc"
[ $rc -eq 0 ] || exit $rc
timeout -s KILL 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/pmc_write -o run --output-format csv -- $BENCH --no-roofline > $OUT/pmc_write.log 2>&1; rc=$?; echo "pmc write rc=$rc"
[ $rc -eq 0 ] || exit $rc
timeout -s KILL 300 rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE -d $OUT/pmc_mfma -o run --output-format csv -- $BENCH --no-roofline > $OUT/pmc_mfma.log 2>&1; rc=$?; echo "pmc mfma rc=$rc"
[ $rc -eq 0 ] || exit $rc
cd $R
python scripts/pmc_traffic.py $OUT/pmc_traffic.json $OUT/pmc_fetch $OUT/pmc_write $OUT/prof $OUT/pmc_mfma $OUT/bench.log > /dev/null; echo "pmc_traffic rc=$?"
f=$(find $OUT/prof -name "*kernel_trace.csv" | head -1)
python scripts/step_critical.py $f 2 > $OUT/crit.txt; head -3 $OUT/crit.txt

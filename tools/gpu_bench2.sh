#!/bin/bash
# kernel+model tests -> bench (with cpu baseline) -> kernel-trace stats -> two PMC passes (FETCH_SIZE, WRITE_SIZE);
# outputs under $WFAE_OUT (default bench_out/)
R=$(cd "$(dirname "$0")/.." && pwd); cd "$R"
O=$R/${WFAE_OUT:-bench_out}; mkdir -p "$O"; export TMPDIR=/tmp
timeout -k 10 1100 python -m pytest tests -m gpu -q --no-header -p no:cacheprovider -x > $O/gpu_tests.log 2>&1
rc=$?; tail -n 5 $O/gpu_tests.log; echo "gpu tests rc=$rc"
if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 600 python bench.py --full --steps 5 --warmup 2 > $O/bench.log 2> $O/bench.err || { tail -30 $O/bench.err; exit 4; }
cat $O/bench.log
cd /tmp && timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-kernel-timing --no-overlap --no-fp32-leg > $O/prof.log 2>&1 || { tail -30 $O/prof.log; exit 5; }
cd /tmp && timeout -k 10 400 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/pmc_fetch -- python3 $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-kernel-timing --no-overlap --no-fp32-leg > $O/pmc_fetch.log 2>&1 || { tail -30 $O/pmc_fetch.log; exit 6; }
cd /tmp && timeout -k 10 400 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/pmc_write -- python3 $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-kernel-timing --no-overlap --no-fp32-leg > $O/pmc_write.log 2>&1 || { tail -30 $O/pmc_write.log; exit 7; }
cd $R && find $O -name "*.csv" | head -20

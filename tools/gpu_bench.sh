#!/bin/bash
# model tests -> smoke -> bench -> rocprofv3 kernel trace of a short bench; outputs under $WFAE_OUT (default bench_out/)
R=$(cd "$(dirname "$0")/.." && pwd); cd "$R"
O=$R/${WFAE_OUT:-bench_out}; mkdir -p "$O"
export TMPDIR=/tmp
timeout -k 10 500 python -m pytest tests/test_model_gpu.py -m gpu -q --no-header -p no:cacheprovider -x > $O/model.log 2>&1
rc=$?; tail -n 15 $O/model.log; echo "model tests rc=$rc"
if [ $rc -gt 1 ]; then exit $rc; fi
timeout -k 10 300 python __graft_entry__.py --smoke > $O/smoke.log 2>&1 || { tail -20 $O/smoke.log; exit 3; }
tail -n 2 $O/smoke.log
timeout -k 10 600 python bench.py --full ${BENCH_ARGS:---steps 5 --warmup 2} > $O/bench.log 2> $O/bench.err || { tail -30 $O/bench.err; exit 4; }
cat $O/bench.log
cd /tmp && timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-kernel-timing > $O/prof.log 2>&1 || { tail -30 $O/prof.log; exit 5; }
cd $R && find $O/prof -name "*stats*" | head; tail -3 $O/prof.log

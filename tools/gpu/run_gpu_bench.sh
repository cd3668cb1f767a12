#!/bin/bash
# GPU bench (the full line: extras + CPU baseline) + profile run. Each GPU step has its own time limit; stop at the
# first failure. Output under $O (default bench_out/).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")}"
O=${O:-bench_out}
mkdir -p $O
export TMPDIR=/tmp
STEPS=${STEPS:-3}
INST=${INST:-1000000}
timeout -k 10 600 python bench.py --full --steps $STEPS --warmup 1 --instances $INST ${BENCH_ARGS} > $O/bench.json 2> $O/bench.err || { echo "bench failed rc=$?"; tail -20 $O/bench.err; exit 1; }
cat $O/bench.json
if [ -n "$PROFILE" ]; then
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $O/prof -o run --output-format csv -- python3 bench.py --steps 2 --warmup 1 --instances $INST --full --no-cpu-baseline > $O/prof_bench.json 2> $O/prof.err || { echo "rocprof failed rc=$?"; tail -20 $O/prof.err; exit 1; }
  find $O/prof -name '*stats*' | head
fi

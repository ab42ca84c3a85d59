#!/bin/bash
# On an MI355X: the -m gpu suite, then bench.py in its plain form (headline
# only) and with --full (every other line; the CPU baseline left out).
# Usage: tools/gpu_check.sh <tag> [outdir]   (outputs under outdir, default check_out/)
set -u
tag=$1
out=${2:-check_out}
mkdir -p $out
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread \
    > $out/${tag}_tests.log 2>&1
rc=$?
tail -3 $out/${tag}_tests.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 120 python -u bench.py --steps 20 --warmup 5 > $out/${tag}_bench_plain.json 2> $out/${tag}_bench_plain.err &&
timeout -k 10 500 python -u bench.py --full --no-cpu-baseline > $out/${tag}_bench_full.json 2> $out/${tag}_bench_full.err

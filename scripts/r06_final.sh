# The round-end gate as the driver runs it (every -m gpu test, smoke), then bench.py --full (CPU
# baseline and live pass ceilings included) -> $O/r06_bench_headline.jsonl (O: OUT_DIR, default out/).
set -o pipefail
export TMPDIR=/tmp
bash scripts/check.sh || exit $?
O=${OUT_DIR:-out}; mkdir -p $O
timeout -k 10 600 python -u bench.py --full > $O/r06_bench.log 2>&1; rc=$?
tail -1 $O/r06_bench.log > $O/r06_bench_headline.jsonl
tail -1 $O/r06_bench.log | cut -c1-300; exit $rc

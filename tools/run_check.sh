# Run on the GPU machine: the whole GPU test suite, then the full bench line (bench.py --full).
# usage: bash tools/run_check.sh OUT_DIR [bench.py args...]  ->  OUT_DIR/{pytest.log,parity_margins.txt,bench.json,bench.err}
set -u
O=$(realpath -m "${1:?usage: run_check.sh OUT_DIR [bench.py args...]}"); shift
cd "$(dirname "$0")/.."
mkdir -p "$O"
rm -f "$O/parity_margins.txt"
FF_PARITY_MARGINS=$O/parity_margins.txt timeout 2400 python -m pytest tests -m gpu -q -x > "$O/pytest.log" 2>&1; echo "pytest rc=$?" >> "$O/pytest.log"
tail -4 "$O/pytest.log"
timeout 900 python bench.py --full "$@" > "$O/bench.json" 2> "$O/bench.err"; tail -c 600 "$O/bench.json"

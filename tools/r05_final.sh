# round-5 final tree: full GPU suite, smoke, the full bench line (logs under $O, default bench_out)
set -o pipefail
P=${1:-r05ap}
O=${O:-bench_out}
mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -q -m gpu --timeout 600 --timeout-method thread > $O/${P}_tests.log 2>&1
rc=$?
tail -3 $O/${P}_tests.log
[ $rc -gt 1 ] && exit 1
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/${P}_smoke.log 2>&1 || exit 1
timeout -k 10 600 python bench.py --full > $O/${P}_bench.json 2> $O/${P}_bench.err || exit 1
exit $rc

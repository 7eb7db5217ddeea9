#!/bin/bash
# round-6 tree check: full GPU suite, smoke, the full bench line (the driver's round-end sequence);
# logs under $O (default bench_out)
#   bash tools/r06_final.sh TAG [bench args...]
set -o pipefail
P=${1:-r06x}; shift
O=${O:-bench_out}
mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -q -m gpu -x --timeout 600 --timeout-method thread > $O/${P}_tests.log 2>&1
rc=$?
tail -3 $O/${P}_tests.log
[ $rc -gt 1 ] && exit 1
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/${P}_smoke.log 2>&1 || exit 1
timeout -k 10 700 python bench.py --full "$@" > $O/${P}_bench.json 2> $O/${P}_bench.err || { echo "bench rc=$?"; tail -5 $O/${P}_bench.err; exit 1; }
python3 -c "import json; d=json.loads(open('$O/${P}_bench.json').read().strip().splitlines()[-1]); print(json.dumps(d['legs']))"
exit $rc

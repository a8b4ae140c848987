#!/bin/bash
# Env sweep of the bench: each argument is one env assignment list ("A=1 B=2"); prints value + stages.
# The bench lines are kept in $OUT (default: a fresh temporary directory).
cd "$(dirname "$0")/.."
O=${OUT:-$(mktemp -d)}
mkdir -p $O
i=0
for cfg in "$@"; do
  env $cfg timeout -k 10 200 python bench.py --full --no-cpu-baseline --steps 10 > $O/b$i.json 2> $O/b$i.err || { echo "FAIL $cfg"; tail -5 $O/b$i.err; exit 1; }
  python3 -c "import json,sys;d=json.load(open(sys.argv[2]));print(sys.argv[1],'|',d['value'],d['ms_per_step'],'|',' '.join('%s=%.0f'%(k,v['avg_us']) for k,v in d['stages'].items()))" "$cfg" $O/b$i.json
  i=$((i+1))
done

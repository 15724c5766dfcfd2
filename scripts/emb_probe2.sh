#!/bin/bash
# development: does the embedded VGICP line depend on what main() ran before it?   scripts/emb_probe2.sh <out-dir>
out=$1; mkdir -p $out
show() { python -c "
import json,sys
d=json.loads(open('$1').read().strip().splitlines()[-1])
e=d['extra']['vgicp']; print('$2', round(e['ms_per_step'],4), round(e['roofline']['target_prep_ms'],4))"; }
python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $out/e1.json 2>/dev/null; show $out/e1.json "steps 2:"
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --map-points 200000 > $out/e2.json 2>/dev/null; show $out/e2.json "map 200k:"
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --scans 2 > $out/e3.json 2>/dev/null; show $out/e3.json "scans 2:"

#!/bin/bash
# round 5: full-batch parity runs of the final code -- EVERY chain of the batch against the oracle (FCZ bytes + coordinates), and the
# first 65 536 chains against the live reference (cpu_baseline sample). Lines land in <out dir>/r5_parity_*.json.
# usage: tools/r5_full_parity.sh <out dir>
OUT=${1:?usage: tools/r5_full_parity.sh <out dir>}; mkdir -p "$OUT"
OFF="--steps 2 --warmup 1 --pdb-sample 0 --mixed-chains 0 --e2e-files 0 --host-chains 0"
python bench.py --full --parity-chains 1000000 --cpu-sample 65536 $OFF > $OUT/r5_parity_1m.json 2> $OUT/r5_parity_1m.err
python bench.py --full --mixed --chains 542000 --parity-chains 542000 --cpu-sample 32768 $OFF > $OUT/r5_parity_mixed_542k.json 2> $OUT/r5_parity_mixed_542k.err
: > $OUT/r5_parity_sweeps.jsonl
python bench.py --full --residues 37 --chains 2000000 --seed-base 11000000000 --parity-chains 2000000 --cpu-sample 65536 $OFF >> $OUT/r5_parity_sweeps.jsonl 2> $OUT/r5_parity_sweeps.err
python bench.py --full --residues 129 --chains 1000000 --seed-base 55000000000 --parity-chains 1000000 --cpu-sample 32768 $OFF >> $OUT/r5_parity_sweeps.jsonl 2>> $OUT/r5_parity_sweeps.err
python bench.py --full --residues 16 --chains 2000000 --seed-base 66000000000 --parity-chains 2000000 --cpu-sample 65536 $OFF >> $OUT/r5_parity_sweeps.jsonl 2>> $OUT/r5_parity_sweeps.err
python bench.py --full --residues 32 --chains 2000000 --seed-base 99000000000 --parity-chains 2000000 --cpu-sample 65536 $OFF >> $OUT/r5_parity_sweeps.jsonl 2>> $OUT/r5_parity_sweeps.err
python bench.py --full --residues 64 --chains 1000000 --seed-base 77000000000 --parity-chains 1000000 --cpu-sample 32768 $OFF >> $OUT/r5_parity_sweeps.jsonl 2>> $OUT/r5_parity_sweeps.err
python bench.py --full --residues 65 --chains 1000000 --seed-base 88000000000 --parity-chains 1000000 --cpu-sample 32768 $OFF >> $OUT/r5_parity_sweeps.jsonl 2>> $OUT/r5_parity_sweeps.err
python - "$OUT" <<'PY'
import json, os, sys
for f in ("r5_parity_1m.json", "r5_parity_mixed_542k.json"):
    d = json.load(open(os.path.join(sys.argv[1], f))); print(f, d["config"]["workload"], round(d["value"] / 1e9, 3), json.dumps(d["parity"]))
for l in open(os.path.join(sys.argv[1], "r5_parity_sweeps.jsonl")):
    if l.startswith("{"):
        d = json.loads(l); print(d["config"]["workload"], round(d["value"] / 1e9, 3), d["ms_per_step"], json.dumps(d["parity"]), json.dumps(d["roofline"]["kernel_ms"]))
PY

#!/bin/bash
# round 5, VERDICT r4 item 5: short-chain workloads, A/B of library variants. usage: tools/r5_short_ab.sh <tag> <lib>...
TAG=$1; shift
OUT=gpurun_out/short_$TAG.txt; : > $OUT
run() { # lib, label, bench args...
  local lib=$1 label=$2; shift 2
  FCZ_HIP_LIB=$PWD/$lib python bench.py --full "$@" --steps 3 --warmup 1 --cpu-sample 0 --pdb-sample 0 --mixed-chains 0 --e2e-files 0 --host-chains 0 > /tmp/ab.json 2> /tmp/ab.err || { echo "$lib $label FAILED" >> $OUT; tail -3 /tmp/ab.err >> $OUT; return; }
  python - "$lib" "$label" >> $OUT <<'PY'
import json, sys
d = json.load(open("/tmp/ab.json")); k = d["roofline"]["kernel_ms"]; p = d.get("parity") or {}
print(sys.argv[1], sys.argv[2], "Gres/s=%.3f" % (d["value"] / 1e9), "step_ms=%.2f" % d["ms_per_step"], " ".join(f"{n.replace('compress_','c_').replace('decompress_','d_')}={v:.3f}" for n, v in k.items()), "parity=%s/%s/%s" % (p.get("chains_checked"), p.get("fcz_bit_exact"), p.get("coords_bit_exact")))
PY
}
for lib in "$@"; do
  run $lib res37 --residues 37 --chains 2000000 --parity-chains 65536
  run $lib mixed --mixed --chains 542000 --parity-chains 16384
  run $lib res350 --chains 262144 --no-parity
done
cat $OUT

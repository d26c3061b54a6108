#!/bin/bash
# A/B of Engine.FC2_LN (es_gemm_nt_ln: fc2 + residual + the next block's LayerNorm 1 in one launch) on one box,
# interleaved: plain bench.py runs of F1 (R rounds, default 3), then C1 and the N = 8 shard (--batch 8), each way.
#   WHAT="f1 c1 n8" picks the workloads; OUT: the folder for the runs' logs (default: a temporary one).
cd "$(dirname "$(readlink -f "$0")")/.." || exit 1
OUT=${OUT:-$(mktemp -d)}; mkdir -p "$OUT"
ms() { python3 -c "import json; print(json.loads([l for l in open('$1') if l.startswith('{')][-1])['ms_per_step'])"; }
run() {  # name, time limit, bench arguments
  local name=$1 lim=$2; shift 2
  for i in $(seq ${R:-3}); do
    for v in 0 1; do
      ENDOSSL_FC2_LN=$v timeout -k 10 $lim python -u bench.py "$@" > "$OUT/fl_${name}_${v}_$i.log" 2>&1 || { tail -5 "$OUT/fl_${name}_${v}_$i.log"; exit 1; }
      echo "$name fc2_ln=$v run $i: $(ms "$OUT/fl_${name}_${v}_$i.log")"
    done
  done
}
for w in ${WHAT:-f1 c1 n8}; do
  case $w in
    f1) run f1 200 --steps 200 --warmup 5 ;;
    c1) run c1 200 --workload c1 --steps 30 --warmup 3 ;;
    n8) run n8 200 --batch 8 --steps 200 --warmup 5 ;;
  esac
done
exit 0

#!/bin/bash
# Generic same-box A/B of two builds of libserhip on the step: interspeech_ser_amd/lib/libserhip_head.so (previous commit, built by hand)
# against the in-tree library.   bash tools/lib_ab.sh [bench.py args...]
# LIB_AB_TRACE=1 keeps the per-launch events and the step decomposition leg on: the lines then end with the `other` class's ms per batch.
set -e
cd "$(dirname "$0")/.."
OUT=gpurun_out/lib_ab.txt
mkdir -p gpurun_out
: > $OUT
LIBD=$PWD/interspeech_ser_amd/lib
NOTRACE=--no-trace; [ -n "$LIB_AB_TRACE" ] && NOTRACE=
pick='import sys,json; d=json.loads([l for l in sys.stdin if l.startswith("{")][-1]); print(d["value"], d["ms_per_step"], d.get("verified"), "other_ms_per_batch", ((d.get("step_decomposition") or {}).get("classes") or {}).get("other", {}).get("ms_per_batch"))'
for rep in 1 2 3; do
for v in head new; do
  L=$LIBD/libserhip_$v.so; [ $v = new ] && L=$LIBD/libserhip.so
  echo "== $v (rep $rep) $*" | tee -a $OUT
  SER_HIP_LIB=$L python bench.py --full --other-encoders none --no-cpu-baseline --no-parity --no-e2e $NOTRACE "$@" 2>/dev/null | python -c "$pick" | tee -a $OUT
done
done

#!/bin/bash
# One lease: the full bench line (bench.py --full: roofline, sub-results, CPU baselines), then the
# forward schedule A/B (in-process, interleaved) for bf16 C2 and the fp8 C2 shape: static
# XCD-paired persistent (default), per-XCD dynamic queues (fwd_dyn=2), and one workgroup per item
# (fwd_persistent=0, the reference's plain grid).
# usage: bash tools/lease_ab.sh <tag> [outdir]     -> <outdir>/<tag>_{bench,ab}.log
set -o pipefail
tag=${1:-lease}
out=${2:-${XFA_EVIDENCE_DIR:-evidence_out}}
mkdir -p "$out"
timeout -k 10 300 python bench.py --full > "$out/${tag}_bench.log" 2>&1 || { tail -5 "$out/${tag}_bench.log"; exit 1; }
tail -1 "$out/${tag}_bench.log" | cut -c1-200
for m in fwd fwd_fp8; do
  timeout -k 10 200 python tools/perf_ab.py --mode $m --rounds 9 --iters 20 --prewarm 2 \
    --var "" --var fwd_dyn=2 --var fwd_persistent=0 >> "$out/${tag}_ab.log" 2>&1 || { tail -5 "$out/${tag}_ab.log"; exit 1; }
done
timeout -k 10 200 python tools/perf_ab.py --mode fwd --noncausal --rounds 5 --iters 10 --prewarm 1 \
  --var "" --var fwd_dyn=2 --var fwd_persistent=0 >> "$out/${tag}_ab.log" 2>&1 || { tail -5 "$out/${tag}_ab.log"; exit 1; }
cat "$out/${tag}_ab.log"

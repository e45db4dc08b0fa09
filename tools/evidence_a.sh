# Evidence call A (one lease): the GPU suite with the parity report and smoke, then the full
# bench line (bench.py --full) and the forward schedule A/B (tools/lease_ab.sh).  Call B:
# tools/pmc_round.sh.
# usage: bash tools/evidence_a.sh <tag>      -> $XFA_EVIDENCE_DIR (default evidence_out)
set -o pipefail
tag=${1:-ev}
out=${XFA_EVIDENCE_DIR:-evidence_out}
mkdir -p "$out"
XFA_PARITY_REPORT="$out/parity.json" timeout -k 10 600 python -u -m pytest tests -m gpu -q --timeout 200 --timeout-method thread > "$out/gpu_suite.log" 2>&1 || { tail -5 "$out/gpu_suite.log"; exit 1; }
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" >> "$out/gpu_suite.log" 2>&1 || { tail -5 "$out/gpu_suite.log"; exit 1; }
tail -3 "$out/gpu_suite.log"
bash tools/lease_ab.sh ${tag} "$out" || exit 1

#!/bin/bash
# Everything the round's committed measurements come from, in one GPU-box call (outputs under OUTDIR).
#   usage: bash tools/round_end_gpu.sh OUTDIR
set -uo pipefail
root="${GRAFT_REPO_ROOT:-$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)}"
cd "$root"
mkdir -p "${1:?usage: bash tools/round_end_gpu.sh OUTDIR}"
out="$(cd "$1" && pwd)"
python -m pytest tests -x -q -m gpu > "$out/pytest_gpu.log" 2>&1; echo "pytest rc=$?" | tee "$out/pytest_rc.txt"
tail -n 3 "$out/pytest_gpu.log"
bash tools/profile.sh final_r06_perf > "$out/profile_perf.log" 2>&1; echo "profile perf rc=$?"
bash tools/profile.sh final_r06_parity --hparams parity > "$out/profile_parity.log" 2>&1; echo "profile parity rc=$?"
export TMPDIR=/tmp
( cd /tmp && RN_PROBE_STEPS=12 RN_PROBE_256=1 RN_PROBE_DEVICE=1 rocprofv3 --kernel-trace -d "$out/train_prof" -o train -- \
  python3 "$root/tools/train_probe.py" perf 32 > "$out/train_probe_device.log" 2>&1 ); echo "train profile rc=$?"
# kernel table + per-step lines, and the launches of the last step (what profiles/rNN/train_step_summary.txt is assembled from)
python3 tools/train_summary.py "$out/train_prof/train_results.db" "$out/train_probe_device.log" > "$out/train_summary.txt" 2>&1
python3 tools/step_trace.py "$out/train_prof/train_results.db" > "$out/train_step_trace.txt" 2>&1
RN_PROBE_STEPS=12 RN_PROBE_256=1 python3 tools/train_probe.py perf 32 > "$out/train_probe_host.log" 2>&1
RN_CONFIG5_FULL=1 python3 tools/run_configs.py > "$out/other_configs.txt" 2> "$out/other_configs.err"; echo "run_configs rc=$?"
python3 tools/spectrum_bench.py > "$out/spectrum_bench.txt" 2>&1; echo "spectrum rc=$?"
python3 bench.py --full > "$out/bench_default.json" 2> "$out/bench_default.err"; echo "bench rc=$?"
tail -n 1 "$out/bench_default.json"

#!/bin/bash
# End-of-round battery on the GPU box (run from the repo root): the GPU suite, the stand-alone fuzz on three seeds,
# the rocprofv3 passes of tools/profile_round.sh on the same binary, a bench.py --full run, and the multi-process rehearsal.
#   bash tools/end_of_round.sh r06 [fuzz seconds per seed] [log directory, default logs]
R=${1:-r06}
FZ=${2:-150}
REPO=${GRAFT_REPO_ROOT:-$PWD}
cd $REPO
LOG=$(realpath -m "${3:-logs}")
mkdir -p "$LOG"
python -m pytest tests -m gpu -q 2>&1 | tail -5 > "$LOG/${R}_pytest_gpu_final.log"
tail -2 "$LOG/${R}_pytest_gpu_final.log"
for S in 0 17 23; do
  python tools/fuzz_parity.py $FZ $S 2>&1 | grep -v amdgpu.ids > "$LOG/${R}_fuzz_seed$S.log"
  tail -1 "$LOG/${R}_fuzz_seed$S.log"
done
bash tools/profile_round.sh $R > "$LOG/${R}_profile_round.log" 2>&1
tail -3 "$LOG/${R}_profile_round.log"
cd $REPO
python bench.py --full --detail "$LOG/${R}_bench_full.json" > "$LOG/${R}_bench_stdout.log" 2> "$LOG/${R}_bench_stderr.log"
tail -1 "$LOG/${R}_bench_stdout.log" > "$LOG/${R}_bench_line.json"
bash tools/rehearse_multi_gpu.sh > "$LOG/${R}_rehearsal_n2_one_gpu.log" 2>&1
tail -1 "$LOG/${R}_rehearsal_n2_one_gpu.log" | cut -c1-400

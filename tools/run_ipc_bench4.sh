#!/bin/bash
# Developer helper (GPU box): bench.py with 4 ranks sharing the one GPU through the hipIpc communicator.
#   EX=ipc|ipc-async SIZE=256 [OUT=<directory for the ranks' lines and logs>] bash tools/run_ipc_bench4.sh
cd ${GRAFT_REPO_ROOT:-$(dirname "$(readlink -f "$0")")/..}
OUT=${OUT:-${TMPDIR:-/tmp}/dfft_ipc_bench4}; mkdir -p "$OUT"
EX=${EX:-ipc}; SIZE=${SIZE:-256}; W=${W:-4}
for ((r = 0; r < W; r++)); do
  RANK=$r LOCAL_RANK=$r WORLD_SIZE=$W MASTER_ADDR=127.0.0.1 MASTER_PORT=${PORT:-29611} DFFT_EXCHANGE=$EX \
    python bench.py --gpus $W --size $SIZE --steps 10 --warmup 3 --full --no-cpu-baseline > "$OUT/bench_${EX}_$r.json" 2> "$OUT/bench_${EX}_$r.err" &
done
wait
cat "$OUT/bench_${EX}_0.json"

set -u
export TMPDIR=/tmp
OUT=${1:?usage: bash scripts/bench_rehearsal.sh OUTDIR}
mkdir -p "$OUT"
# each step under its own time limit; the first non-zero status ends the script before another GPU process starts
NBX_BENCH_FORCE_DIST=1 timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29541 bench.py --gpus 1 --bodies 1048576 --steps 10 --warmup 2 --full > "$OUT/bench_rehearsal_1rank_rccl_1m.json" 2> "$OUT/bench_rehearsal_1rank.err" || { echo rc1=$?; exit 1; }
NBX_BENCH_BACKEND=gloo timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29543 bench.py --gpus 2 --steps 6 --warmup 2 --cpu-baseline none --full > "$OUT/bench_rehearsal_2ranks_one_gpu_gloo.json" 2> "$OUT/bench_rehearsal_2ranks.err" || { echo rc2=$?; exit 1; }
NBX_BENCH_BACKEND=gloo timeout -k 10 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node 4 --master-addr 127.0.0.1 --master-port 29545 bench.py --gpus 4 --steps 6 --warmup 2 --cpu-baseline none --full > "$OUT/bench_rehearsal_4ranks_one_gpu_gloo.json" 2> "$OUT/bench_rehearsal_4ranks.err" || { echo rc3=$?; exit 1; }
tail -c 1500 "$OUT/bench_rehearsal_1rank_rccl_1m.json"

# Two ranks on the one GPU of a gpurun box over gloo: rehearses bench.py's multi-rank path
# (torchrun env, barriers, max-over-ranks timing, obs all-gather); the RCCL run is the driver's.
# Output: $OUT_DIR/dist/ (default bench_out/dist/).
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
OUT=${OUT_DIR:-bench_out}/dist
mkdir -p $OUT
timeout -k 10 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 2 --steps 64 --warmup 16 --full --dist-backend gloo > $OUT/bench2.json 2> $OUT/bench2.err
echo "rc=$?" >> $OUT/bench2.err

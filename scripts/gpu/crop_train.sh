#!/bin/bash
# crop_train.sh: train.py on a generated mixed-size JPEG set (the protocol of ragged_train.sh), whole images at batch 1
# against random 384x512 crops at batch 8 with 1 and 4 crops per decoded image, the three arms interleaved twice in one
# session; then the step alone (bench.py) at the crop's shape and the crop / resize launch times.
# usage: crop_train.sh OUT_DIR (JSONL and logs go there).  Every step runs under its own time limit; a failing step ends the session.
cd "$(dirname "$0")/../.." || exit 2
export TMPDIR=/tmp
O=${1:?usage: crop_train.sh OUT_DIR}
mkdir -p $O
timeout -k 10 300 python scripts/make_jpeg_set.py --root /tmp/sha_mixed --train 160 --test 16 --mixed --workers 12 > $O/mk.log 2>&1 || exit $?
T="python train.py --epochs 5 --eval-every 100 --show False --wandb False --num-workers 12 --seed 0 --data_root /tmp/sha_mixed"
for rep in 1 2; do
  timeout -k 10 240 $T --batch-size 1 --checkpoint-dir /tmp/ck_a$rep --log-jsonl $O/train_mixed_b1_$rep.jsonl > $O/a$rep.log 2>&1 || exit $?
  timeout -k 10 240 $T --batch-size 8 --crop-size 384x512 --checkpoint-dir /tmp/ck_b$rep --log-jsonl $O/train_crop_b8_k1_$rep.jsonl > $O/b$rep.log 2>&1 || exit $?
  timeout -k 10 240 $T --batch-size 8 --crop-size 384x512 --crops-per-image 4 --checkpoint-dir /tmp/ck_c$rep --log-jsonl $O/train_crop_b8_k4_$rep.jsonl > $O/c$rep.log 2>&1 || exit $?
done
timeout -k 10 200 python bench.py --steps 20 --warmup 5 --batch 8 --height 384 --width 512 > $O/bench_b8.log 2>&1 || exit $?
timeout -k 10 200 python bench.py --steps 20 --warmup 5 --batch 32 --height 384 --width 512 > $O/bench_b32.log 2>&1 || exit $?
grep -h '"metric"' $O/bench_b8.log $O/bench_b32.log > $O/bench_384x512.jsonl
timeout -k 10 120 python scripts/prof/crop_launch_time.py > $O/crop_launch_time.jsonl 2> $O/crop_launch_time.err || exit $?
grep -h '"kind": "epoch"' $O/train_*.jsonl | cut -c1-400
cat $O/bench_384x512.jsonl $O/crop_launch_time.jsonl
echo done

#!/bin/bash
# heads_train.sh: train.py on the generated mixed-size JPEG set with head sidecars (scripts/make_jpeg_set.py --mixed
# --heads, the protocol of profiles/r13/scale_train.sh): random 384x512 crops at batch 8, --crop-scale 0.75,1.33, with
# 1 and 4 crops per decoded image, each with and without --gt-from-heads, the four arms interleaved twice in one
# session; then the launch times.
# usage: heads_train.sh OUT_DIR (JSONL and logs go there), from the repository root.  Every step runs under its own
# time limit; a failing step ends the session.
export TMPDIR=/tmp
O=${1:?usage: heads_train.sh OUT_DIR}
HERE=$(dirname "$0")
mkdir -p $O
timeout -k 10 300 python scripts/make_jpeg_set.py --root /tmp/sha_mixed_heads --train 160 --test 16 --mixed --heads --workers 12 > $O/mk.log 2>&1 || exit $?
T="python train.py --epochs 5 --eval-every 100 --show False --wandb False --num-workers 12 --seed 0 --data_root /tmp/sha_mixed_heads --batch-size 8 --crop-size 384x512 --crop-scale 0.75,1.33"
for rep in 1 2; do
  timeout -k 10 240 $T --checkpoint-dir /tmp/ck_a$rep --log-jsonl $O/train_map_b8_k1_$rep.jsonl > $O/a$rep.log 2>&1 || exit $?
  timeout -k 10 240 $T --gt-from-heads --checkpoint-dir /tmp/ck_b$rep --log-jsonl $O/train_heads_b8_k1_$rep.jsonl > $O/b$rep.log 2>&1 || exit $?
  timeout -k 10 240 $T --crops-per-image 4 --checkpoint-dir /tmp/ck_c$rep --log-jsonl $O/train_map_b8_k4_$rep.jsonl > $O/c$rep.log 2>&1 || exit $?
  timeout -k 10 240 $T --crops-per-image 4 --gt-from-heads --checkpoint-dir /tmp/ck_d$rep --log-jsonl $O/train_heads_b8_k4_$rep.jsonl > $O/d$rep.log 2>&1 || exit $?
done
timeout -k 10 240 python $HERE/gt_launch_time.py > $O/gt_launch_time.jsonl 2> $O/gt_launch_time.err || exit $?
grep -h '"kind": "epoch"' $O/train_*.jsonl | cut -c1-400
cat $O/gt_launch_time.jsonl
echo done

#!/bin/bash
# roi_train.sh: the launch times (roi_launch_time.py), then train.py on the generated mixed-size JPEG set (the protocol
# of profiles/r13/scale_train.sh): random 384x512 crops at batch 8 with --crop-scale 0.75,1.33, 1 and 4 crops per
# decoded image, each with and without --roi-masks, the four arms interleaved twice in one session.
# usage: roi_train.sh OUT_DIR (JSONL and logs go there), from the repository root.  Every step runs under its own
# time limit; a failing step ends the session.
export TMPDIR=/tmp
O=${1:?usage: roi_train.sh OUT_DIR}
HERE=$(dirname "$0")
mkdir -p $O
timeout -k 10 120 python $HERE/roi_launch_time.py > $O/roi_launch_time.jsonl 2> $O/roi_launch_time.err || exit $?
cat $O/roi_launch_time.jsonl
timeout -k 10 300 python scripts/make_jpeg_set.py --root /tmp/sha_mixed --train 160 --test 16 --mixed --workers 12 > $O/mk.log 2>&1 || exit $?
timeout -k 10 120 python $HERE/make_roi_masks.py /tmp/sha_mixed >> $O/mk.log 2>&1 || exit $?
T="python train.py --epochs 5 --eval-every 100 --show False --wandb False --num-workers 12 --seed 0 --data_root /tmp/sha_mixed --batch-size 8 --crop-size 384x512 --crop-scale 0.75,1.33"
for rep in 1 2; do
  timeout -k 10 240 $T --checkpoint-dir /tmp/ck_a$rep --log-jsonl $O/train_plain_b8_k1_$rep.jsonl > $O/a$rep.log 2>&1 || exit $?
  timeout -k 10 240 $T --roi-masks --checkpoint-dir /tmp/ck_b$rep --log-jsonl $O/train_roi_b8_k1_$rep.jsonl > $O/b$rep.log 2>&1 || exit $?
  timeout -k 10 240 $T --crops-per-image 4 --checkpoint-dir /tmp/ck_c$rep --log-jsonl $O/train_plain_b8_k4_$rep.jsonl > $O/c$rep.log 2>&1 || exit $?
  timeout -k 10 240 $T --roi-masks --crops-per-image 4 --checkpoint-dir /tmp/ck_d$rep --log-jsonl $O/train_roi_b8_k4_$rep.jsonl > $O/d$rep.log 2>&1 || exit $?
done
grep -h '"kind": "epoch"' $O/train_*.jsonl | cut -c1-400
echo done

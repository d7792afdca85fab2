#!/bin/bash
# Per-kernel durations of the bf16 ViT in one launch form: a `rocprofv3 --kernel-trace --stats` run of its own.
#   tools/vit_bf16_form_prof.sh B [form] [OUT.txt]     (form: few_frame | small | throughput | default)
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd); B=${1:-1}; FORM=${2:-few_frame}; OUT=${3:-$ROOT/profiles/vit_bf16_${FORM}_B${B}_kernel_stats.txt}
D=$(mktemp -d)
rocprofv3 --kernel-trace --stats -d $D -o prof --output-format csv -- python $ROOT/tools/vit_bf16_form_run.py $B $FORM > $D/run.log 2>&1 || { tail -20 $D/run.log; exit 1; }
mkdir -p "$(dirname "$OUT")"
python $ROOT/tools/kstats.py $D 14 > $OUT; cat $OUT

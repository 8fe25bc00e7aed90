#!/bin/bash
# Interleaved bench lines of whole source trees (each with its own built library) on one box.
# Usage: bash tools/ab_trees.sh <workload> <reps> <steps> <tree dir>...   ("." = this tree)
# The trees may predate bench.py --full, so the plain line is taken: the time per step is the
# roofline block's kernel average where a tree prints one, its ms_per_step otherwise.
W=$1; R=$2; S=$3; shift 3
ROOT=$PWD
O=$ROOT/ab; mkdir -p $O
for rep in $(seq $R); do
  for T in "$@"; do
    (cd $T && timeout -k 10 180 python bench.py --workload $W --steps $S --warmup 20 --no-cpu-baseline > $O/abt.json) || exit 1
    python -c "import json; d=json.load(open('$O/abt.json')); us=d.get('roofline', {}).get('avg_kernel_us', d['ms_per_step'] * 1e3); print('$W $T', f\"{d['value']/1e6:.2f}M\", f\"step {us:.1f}us\")"
  done
done

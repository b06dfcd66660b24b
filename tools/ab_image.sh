#!/bin/bash
# tools/ab.sh for the image-only launch: two builds of the library on ONE box, alternating rounds, the image-only K_A and the step at
# cfg2 with rotated input and with one buffer (tools/ka_image_time.py).  usage: tools/ab_image.sh <libA.so> <libB.so> [rounds] [launches per batch]
A=$1; B=$2; N=${3:-5}; IT=${4:-60}
cd "$(dirname "$0")/.."
for r in $(seq 1 $N); do
  for L in "$A" "$B"; do
    echo -n "$(basename $L): "
    SGZ_LIB=$(pwd)/$L timeout -k 10 120 python tools/ka_image_time.py $IT 2>&1 | tail -1 | python -c "
import ast,sys
d=ast.literal_eval(sys.stdin.read())
print(' | '.join(f\"{k} K_A {v['ka_us']:.2f}/{v['ka_min_us']:.2f} step {v['step_us']:.2f}/{v['step_min_us']:.2f}\" for k,v in d.items()))" || exit 1
  done
done

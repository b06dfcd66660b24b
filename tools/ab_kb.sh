#!/bin/bash
# tools/ab.sh for K_B alone: any number of builds of the library on ONE box, alternating rounds of tools/kb_time.py (K_B on precomputed
# magnitudes at cfg2).  Of the two lines kb_time.py prints, the last is recorded: image only, and with lines + state.
# The first run that fails -- any non-zero status of kb_time.py or of its time limit (124 / 137), an abort (134) and a segmentation
# fault (139) included -- ends the script: nothing more is started on the device behind it.
# usage: tools/ab_kb.sh <rounds> <launches per batch> <libA.so> <libB.so> ...
set -o pipefail
N=$1; IT=$2; shift 2
cd "$(dirname "$0")/.."
for r in $(seq 1 $N); do
  for L in "$@"; do
    out=$(SGZ_LIB=$(pwd)/$L timeout -k 10 120 python tools/kb_time.py $IT 2>&1)
    rc=$?
    if [ $rc -ne 0 ]; then
      echo "round $r $(basename $L): kb_time.py ended with status $rc; stopping"
      echo "$out" | tail -5
      exit $rc
    fi
    echo "round $r $(basename $L): $(echo "$out" | tail -1)"
  done
done

#!/bin/bash
# The release kernels with the one-round schedule's knobs at run time (-DSGZ_SCHED_SWEEP without -DSGZ_DEBUG: no stamps, no phase clocks;
# sgz_debug_set_schedule, sgz_debug_set_priorities) -> tools/ab/lib_sweep.so, for tools/image_sched_sweep.py: spectrum_real.hip and api.hip
# recompiled with the flag, linked with the current objects of the other translation units.
# usage: tools/mksweep.sh [extra hipcc flags ...]
set -e
cd "$(dirname "$0")/.."
B=signalizer_amd/build
python signalizer_amd/build.py > /dev/null
mkdir -p tools/ab
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fhip-fp32-correctly-rounded-divide-sqrt -x hip -DSGZ_SCHED_SWEEP"
/opt/rocm/bin/hipcc $F -fno-slp-vectorize -c signalizer_amd/csrc/spectrum_real.hip -o tools/ab/sweep_real.o "$@" &
/opt/rocm/bin/hipcc $F -c signalizer_amd/csrc/api.hip -o tools/ab/sweep_api.o "$@" &
wait
OBJS=$(ls $B/*.o | grep -v "/spectrum_real.hip.o" | grep -v "/api.hip.o")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/ab/lib_sweep.so $OBJS tools/ab/sweep_real.o tools/ab/sweep_api.o -ldl
echo tools/ab/lib_sweep.so

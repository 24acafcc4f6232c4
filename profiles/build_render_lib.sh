#!/bin/bash
# profiles/build_render_lib.sh NAME "FLAGS": icon-ray-tracing_amd/libicon_rt_hip_NAME.so, the
# product library (make lib) with the raygen (irt_render.hip and its two headers) rebuilt under
# extra compiler flags, for an A/B of code generation (e.g. "-mllvm -amdgpu-schedule-metric-bias=5").
# The build macros it was written for (the held-argument forms of the raygen) are gone from the
# source: without a define of your own it only repeats the Makefile's RENDER_FLAGS build.  Run on
# the CPU host after `make lib`; the library is loaded through IRT_LIB_PATH.
set -e
NAME=${1:?name}; DEFS=${2:?flags}
P=$(cd "$(dirname "$0")/../icon-ray-tracing_amd" && pwd)
X=$P/build-x-$NAME
mkdir -p $X
/opt/rocm/bin/hipcc -std=c++17 -O3 --offload-arch=gfx950 -ffp-contract=off -fno-fast-math \
  -fhip-fp32-correctly-rounded-divide-sqrt -fPIC -Wall -I$P/../include -I$P/csrc -I$P/host -D__HIP_PLATFORM_AMD__ \
  -mllvm -amdgpu-load-store-vectorizer=0 $DEFS -c $P/csrc/irt_render.hip -o $X/irt_render.o
B=$P/build
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $P/libicon_rt_hip_$NAME.so $B/irt_host.o $B/irt_scene.o \
  $B/irt_synth.o $B/irt_debug.o $B/irt_netcdf.o $B/irt_convert.o $B/irt_sched.o $B/irt_kernels.o $X/irt_render.o \
  $B/irt_context.o $B/irt_launch.o $B/irt_debug_hooks.o $B/irt_build.o -lpthread

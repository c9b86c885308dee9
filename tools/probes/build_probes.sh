#!/bin/bash
# Probe builds for tools/coresidency_bisect.py: small libraries of ac_mdx.hip built WITH packed float32 (no NOPK flags) + ac_api (context,
# error string), and the canary kernels.
# Run from the repo root after `make -C audio_cut_amd/csrc`; outputs under tools/probes/build/ (git-ignored, shipped by gpurun).
set -e
cd "$(dirname "$0")/../../audio_cut_amd/csrc"
OUT=../../tools/probes/build
mkdir -p $OUT /tmp/probe_objs
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function -Wno-unused-variable -Wno-unused-but-set-variable -ffp-contract=off"
build() {  # name source extra-flags
  /opt/rocm/bin/hipcc $FLAGS $3 -c $2 -o /tmp/probe_objs/$1.o && /opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 /tmp/probe_objs/$1.o build/ac_api.o -o $OUT/lib$1.so
}
build mdx_pk ac_mdx.hip "" &
build mdx_nopk ac_mdx.hip "-Xclang -target-feature -Xclang -packed-fp32-ops" &
build mdx_noslp ac_mdx.hip "-fno-slp-vectorize" &
wait
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -shared -fPIC ../../tools/probes/canary.hip -o $OUT/libcanary.so
ls -la $OUT

#!/bin/bash
# Build A/B variants of the product library into build/ab/ (cross-compiled here; build/ travels to the GPU box):
#   tools/ab_build.sh "k1htime:-DK1H_TIMING=1"      then, on the GPU:   FOSPHOR_AMD_LIB=$PWD/build/ab/lib_k1htime.so FOSPHOR_AMD_K1_TIMING=1 python3 tools/k1h_phase_timing.py
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$ROOT/build/ab"
CSRC=$ROOT/gr-fosphor_amd/csrc
for spec in "$@"; do
	name=${spec%%:*}; flags=${spec#*:}
	hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -std=c++17 -fPIC -pthread -Wno-unused-function $flags -x hip -shared \
		-o "$ROOT/build/ab/lib_$name.so" $CSRC/fosphor_kernels.hip $CSRC/fosphor_cmap.hip $CSRC/fosphor_api.cpp $CSRC/fosphor_shard.cpp $CSRC/fosphor_prof.cpp $CSRC/fosphor_tables.cpp $CSRC/fosphor_render.cpp \
		$CSRC/fosphor_sink.cpp $CSRC/fosphor_exchange.cpp -ldl 2>&1 | grep -E "error|spill" || true &
done
wait
ls -la "$ROOT/build/ab/"

#!/bin/bash
# tuning builds of ONE kernel file, or of the few that share a macro: [FILE="fused_voice.hip"] tools/build_variant.sh <name> [-D...]
#   ->  scratch/variants/lib_<name>.so
# (same ABI, loaded with SIG_LIB_PATH; for fused_voice.hip -DSIG_TUNE_SINE_ONLY restricts the template instantiations
# to what tools/tune_kernels.py launches -- that unit alone, Sine kernels, stereo bus -- so a variant builds in seconds;
# the kernels themselves are in sig_fused_walk.h / sig_fused_steady.h / sig_fused_scan.h)
# The voice-program interpreter's kernels are one family per file: FILE="$(cd signals_amd/csrc && echo vp_*.hip)" rebuilds them all
# with -DSIG_VP_WAVES=.. / -DSIG_VP_WAVES1=.. / -DSIG_VP_ROWS=.., FILE=vp_plain.hip the one family a measurement launches.
set -euo pipefail
cd "$(dirname "$0")/../signals_amd/csrc"
name=$1; shift
mkdir -p ../../scratch/variants
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
built=()
skip=()
for file in ${FILE:-fused_voice.hip}; do
  stem=${file%.hip}
  $HIPCC --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -Wno-unused-function "$@" \
      -c "$file" -o ../../scratch/variants/${stem}_$name.o &
  built+=(../../scratch/variants/${stem}_$name.o)
  skip+=("$stem.o")
done
wait
objs=$(ls *.o | grep -v -x -F "$(printf '%s\n' "${skip[@]}")")
for o in "${built[@]}"; do [ -f "$o" ] || { echo "build_variant.sh: $o was not built" >&2; exit 1; }; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o ../../scratch/variants/lib_$name.so "${built[@]}" $objs
echo "built scratch/variants/lib_$name.so"

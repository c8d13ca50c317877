#!/bin/bash
# Builds libsunerf_hip.so (gfx950) in-tree.  Usage: ./build.sh [extra hipcc flags]
set -e
cd "$(dirname "$0")"
OUT=${SUNERF_BUILD_OUT:-../libsunerf_hip.so}     # variants for A/B runs: SUNERF_BUILD_OUT=... SUNERF_BUILD_OBJ=... ./build.sh -DFLAG
OBJ=${SUNERF_BUILD_OBJ:-../build_obj}
mkdir -p "$OBJ"
COMMON="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-result"
# Every source is named once, in one of two lists; both the compile and the link go by them (the link in this order, the AGPR
# objects after train_step.o).
# -amdgpu-mfma-vgpr-form: MFMA accumulators in architectural VGPRs.  The render / dgrad kernels keep their activation
# fragments in the AGPR half of the register file (see render_fwd.hip), so this removes a v_accvgpr_read per accumulator
# element from every tile epilogue.  wgrad.hip holds 256 accumulator registers per lane and wants them in AGPRs.
VGPR_FORM="pack sampler rays columns render_fwd render_bwd dt dt_response_set dem dem_inversion mhd thomson polarimetry train_step bwd_exact metrics observations reprojection volume grid_field dynamic_grid prep instrument patch likelihood ssim_loss deconvolve psf_grad despike coalign stack noise_gate register enhance"
AGPR="wgrad bwd_pipe"     # accumulators in AGPRs (bwd_pipe.hip: 128 per weight-gradient wave, W^T fragments per data-gradient wave)
pids=()
objs=()
for f in $VGPR_FORM; do
  hipcc $COMMON -mllvm -amdgpu-mfma-vgpr-form=1 "$@" -c -o "$OBJ/$f.o" "$f.hip" &
  pids+=($!)
  objs+=("$OBJ/$f.o")
  if [ "$f" = train_step ]; then
    for g in $AGPR; do
      hipcc $COMMON "$@" -c -o "$OBJ/$g.o" "$g.hip" &
      pids+=($!)
      objs+=("$OBJ/$g.o")
    done
  fi
done
for p in "${pids[@]}"; do wait "$p"; done     # set -e: a failed compile fails the build
hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT" "${objs[@]}"
echo "built $OUT"

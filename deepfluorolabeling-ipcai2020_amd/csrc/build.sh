#!/bin/bash
# Builds libdfl_hip.so for gfx950 (cross-compiles without a GPU).  Usage: csrc/build.sh [extra hipcc flags]
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
out="$here/../lib"
mkdir -p "$out"
srcs=(api.hip conv_gemm.hip conv_plan.hip conv_rows.hip convp_bf16.hip convq_bf16.hip convn_bf16.hip convs.hip wgradp_bf16.hip wgrad_gemm.hip direct_small.hip bn_elem.hip head.hip loss.hip prep.hip augment.hip upsample.hip overlay.hip overlay_fullres.hip mesh.hip decimate.hip preproc.hip drr.hip drr_grad.hip sim.hip sim_patch.hip sim_outline.hip sim_mi.hip expose.hip drr_tools.hip raster.hip labels.hip labels_dist.hip boundary.hip ce_loss.hip)
objs=()
pids=()
# one hipcc per source, at most $MAX_JOBS (default 16) at a time
jobs_max="${MAX_JOBS:-16}"
[[ "$jobs_max" =~ ^[1-9][0-9]*$ ]] || jobs_max=16
for s in "${srcs[@]}"; do
  o="$out/${s%.hip}.o"
  objs+=("$o")
  stale=0
  if [ ! -f "$o" ]; then stale=1; fi
  # any header may reach any source: an object is stale when its source or any *.h here or the C API is newer
  for d in "$here/$s" "$here"/*.h "$here/../../include/dfl_hip.h"; do
    if [ "$d" -nt "$o" ]; then stale=1; fi
  done
  if [ "$stale" = 1 ]; then
    # the two patch-resident kernels live at 1-3 waves per SIMD: schedule them for instruction-level parallelism instead of
    # register pressure (same instructions, same results; measured 4.47 -> 4.45 ms per step), and so are the streaming kernels of
    # bn_elem.hip (the batched sums issue their loads earlier: 0.23 -> 0.21 ms per step)
    extra=""
    case "$s" in convp_bf16.hip|convq_bf16.hip|convn_bf16.hip|convs.hip|wgradp_bf16.hip|bn_elem.hip) extra="-mllvm -amdgpu-sched-strategy=max-ilp";; esac
    # the augmentation rounds every product and sum separately, as its numpy restatement (tests/aug_ref.py) does, and the
    # overlays as torch's CPU ops do (an FMA moves results across the 8-bit truncation boundaries)
    # (so does the detector model, as tests/expose_ref.py does, the rasteriser, as tests/raster_ref.py does, and the
    # decimation, as tests/decimate_ref.py does, and the tool chords, as tests/tools_ref.py does, and the bins and Parzen
    # weights of the mutual-information cost, as tests/mi_ref.py does)
    case "$s" in augment.hip|overlay.hip|overlay_fullres.hip|expose.hip|drr_tools.hip|raster.hip|decimate.hip|sim_mi.hip) extra="-ffp-contract=off";; esac
    if [ "${#pids[@]}" -ge "$jobs_max" ]; then
      wait "${pids[0]}"
      pids=("${pids[@]:1}")
    fi
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $extra "$@" -c "$here/$s" -o "$o" &
    pids+=($!)
  fi
done
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait "$p"; done
hipcc --offload-arch=gfx950 -shared -fPIC -o "$out/libdfl_hip.so" "${objs[@]}"
echo "built $out/libdfl_hip.so"

#!/bin/bash
# Build libtsu_hip.so for gfx950 in-tree (the .so travels to the GPU box with the repo snapshot).
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="$HERE/../tsu/_lib"
mkdir -p "$OUT" "$HERE/_obj"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function"
objs=()
pids=()
for src in "$HERE"/*.hip; do
    obj="$HERE/_obj/$(basename "${src%.hip}").o"
    objs+=("$obj")
    if [ ! -f "$obj" ] || [ "$src" -nt "$obj" ] || [ "$HERE/tsu_common.h" -nt "$obj" ] || [ "$HERE/ising2d.h" -nt "$obj" ] || [ "$HERE/dense.h" -nt "$obj" ] || [ "$HERE/dense_dev.h" -nt "$obj" ] || [ "$HERE/dense_plan.h" -nt "$obj" ] || [ "$HERE/uf_dev.h" -nt "$obj" ] || [ "$HERE/sw_dev.h" -nt "$obj" ] || [ "$HERE/sw_host.h" -nt "$obj" ] || [ "$HERE/ising2d_pt.h" -nt "$obj" ] || [ "$HERE/ising3d.h" -nt "$obj" ] || [ "$HERE/disorder_dev.h" -nt "$obj" ] || [ "$HERE/pt_dev.h" -nt "$obj" ] || [ "$HERE/pt_host.h" -nt "$obj" ] || [ "$HERE/pt_ladder.h" -nt "$obj" ] || [ "$HERE/reduce_dev.h" -nt "$obj" ] || [ "$HERE/corr_dev.h" -nt "$obj" ] || [ "$HERE/pop_dev.h" -nt "$obj" ] || [ "$HERE/pop_host.h" -nt "$obj" ] || [ "$HERE/link_dev.h" -nt "$obj" ] || [ "$HERE/pte_host.h" -nt "$obj" ] || [ "$HERE/sparse_host.h" -nt "$obj" ] || [ "$HERE/sparse.h" -nt "$obj" ] || [ "$HERE/sparse_batch_dev.h" -nt "$obj" ] || [ "$HERE/../../include/tsu_hip_ensemble.h" -nt "$obj" ] || [ "$HERE/../../include/tsu_hip_sparse_batch.h" -nt "$obj" ] || [ "$HERE/../../include/tsu_hip_overlap.h" -nt "$obj" ] || [ "$HERE/../../include/tsu_hip_population.h" -nt "$obj" ] || [ "$HERE/../../include/tsu_hip_correlation.h" -nt "$obj" ] || [ "$HERE/../../include/tsu_hip.h" -nt "$obj" ] || [ "$HERE/../../include/tsu_hip_ising3d_cluster.h" -nt "$obj" ] || [ "$HERE/../../include/tsu_hip_probe.h" -nt "$obj" ] || [ "$HERE/../../include/tsu_hip_cluster_field.h" -nt "$obj" ] || [ "$HERE/multispin_dev.h" -nt "$obj" ] || [ "$HERE/../../include/tsu_hip_multispin.h" -nt "$obj" ] || [ "$HERE/multispin_host.h" -nt "$obj" ] || [ "$HERE/../../include/tsu_hip_multispin_pt.h" -nt "$obj" ] || [ "$HERE/../../include/tsu_hip_multispin_corr.h" -nt "$obj" ] || [ "$HERE/../../include/tsu_hip_multispin_quench.h" -nt "$obj" ] || [ "$HERE/../../include/tsu_hip_cluster_measure.h" -nt "$obj" ] || [ "$HERE/potts_dev.h" -nt "$obj" ] || [ "$HERE/../../include/tsu_hip_potts.h" -nt "$obj" ] || [ "$HERE/potts_kern_dev.h" -nt "$obj" ] || [ "$HERE/potts_host.h" -nt "$obj" ] || [ "$HERE/../../include/tsu_hip_potts3d.h" -nt "$obj" ] || [ "$HERE/potts_muca_dev.h" -nt "$obj" ] || [ "$HERE/../../include/tsu_hip_potts_muca.h" -nt "$obj" ] || [ "$HERE/potts_disorder_dev.h" -nt "$obj" ] || [ "$HERE/potts_disorder_kern_dev.h" -nt "$obj" ] || [ "$HERE/../../include/tsu_hip_potts_disorder.h" -nt "$obj" ] || [ "$HERE/potts_pt_kern_dev.h" -nt "$obj" ] || [ "$HERE/../../include/tsu_hip_potts_pt.h" -nt "$obj" ] || [ "$HERE/potts_pop_plan.h" -nt "$obj" ] || [ "$HERE/potts_pop_kern_dev.h" -nt "$obj" ] || [ "$HERE/../../include/tsu_hip_potts_pop.h" -nt "$obj" ]; then
        $HIPCC $FLAGS ${TSU_EXTRA_FLAGS:-} -c "$src" -o "$obj" &
        pids+=($!)
    fi
done
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait "$p"; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o "$OUT/libtsu_hip.so.tmp$$" "${objs[@]}"
mv "$OUT/libtsu_hip.so.tmp$$" "$OUT/libtsu_hip.so"
echo "built $OUT/libtsu_hip.so"

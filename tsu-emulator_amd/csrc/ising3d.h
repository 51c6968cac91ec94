// ising3d.h -- the 3-D lattice handle shared by ising3d.hip (heat-bath sweeps, reductions, tempering ladders) and
// ising3d_cluster.hip (Swendsen-Wang cluster steps).
#pragma once
#include "tsu_common.h"

struct tsu_ising3d {
    tsu_ctx* ctx;
    int depth, rows, cols;
    int pz, pr, pc;      // periodic flag per axis
    size_t pitch;        // elements per row, spins and disorder alike (cols rounded up to 16)
    int8_t* s;           // (depth * rows) x pitch spins, pad bytes 0
    float* d_dis;        // J_right, J_down, J_layer, h: four planes of (depth * rows) x pitch fp32, pads 0 (first set_disorder)
    int have_disorder;
    int have_field;      // some stored h is nonzero (set_disorder; a NULL h counts as zero field)
    double* d_part;      // energy: per-workgroup partials + the total
    long long* d_acc;    // sum of spins / overlap accumulator
    unsigned long long launches;  // k8_sweep launches so far
    int32_t* d_labels;   // cluster labels, depth * rows * cols int32, allocated by the first cluster call on the tiled route
    size_t labels_cap;
    void* d_sw_batch;    // tsu_ising3d_cluster_sweep_batch: device copy of the per-lattice items (lives with its first lattice)
    size_t sw_batch_cap;
    int* h_err;          // host-mapped flag: 2 = a capped union / find loop of a cluster kernel expired (results invalid)
    unsigned long long sw_launches;  // cluster-kernel launches so far (not counted in `launches`)
    long long* d_prof;   // tsu_ising3d_profiles: depth + rows + cols int64 bins (first call)
};

// ising3d_cluster.hip: report (and clear) a flag a cluster kernel left in h_err; release what the cluster calls allocated
int ising3d_check_err(tsu_ising3d* L);
void ising3d_cluster_free(tsu_ising3d* L);

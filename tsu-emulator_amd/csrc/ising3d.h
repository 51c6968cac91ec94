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
    tsu_sw_scratch sw;   // cluster steps: labels, batch items, launches (not counted in `launches`)
    int* h_err;          // host-mapped flag: 2 = a capped union / find loop of a cluster kernel expired (results invalid)
    long long* d_prof;   // tsu_ising3d_profiles: depth + rows + cols int64 bins (first call)
};

// ising3d_cluster.hip: report (and clear) a flag a cluster kernel left in h_err
int ising3d_check_err(tsu_ising3d* L);

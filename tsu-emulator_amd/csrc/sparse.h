// sparse.h -- the tsu_sparse handle (K5), shared by sparse.hip, which owns it, and sparse_batch.hip, whose walker batches borrow its
// position-space CSR arrays.
#pragma once
#include <vector>

#include "dense.h"
#include "sparse_host.h"

struct tsu_sparse {
    tsu_ctx* ctx;
    int n, n_colors;
    std::vector<int> color_off;  // host copy
    int64_t* row_ptr;   // n+1, position space
    int32_t* col;       // neighbour POSITIONS, in ascending order of the neighbours' site numbers
    double* val;
    double* bias;       // position space
    int32_t* site_of;   // position -> site
    int32_t* pos_of;    // site -> position
    int8_t* state;      // position space, {0,1}
    int8_t* staging;    // n bytes: site-order image for set/get
    int8_t* samples;    // recorded states (site order)
    size_t samples_cap;
    double* d_red;      // [energy, sum_spins as double pair] reduction target
    int64_t nnz;
    // regular colour classes (k5_stencil): see K5Stencil
    std::vector<K5Stencil> stencil;  // one per colour; deg < 0: the class is not regular
    unsigned long long* d_thr;              // [n_colors][K5_MAX_DEG + 1] acceptance thresholds of the current call
    uint8_t* d_code;                        // [n] (position space) decisions prepared for the second class of a PAIR, see K5Stencil::pair
};

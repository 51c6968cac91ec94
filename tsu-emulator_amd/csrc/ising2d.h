// ising2d.h -- lattice handle shared by ising2d.hip (generic kernel, K4, host API) and ising2d_tiled.hip.
#pragma once
#include "tsu_common.h"

struct tsu_ising2d {
    tsu_ctx* ctx;
    int64_t total_rows;  // global lattice height
    int64_t row0;        // global index of owned row 0
    int rows, cols;      // owned rows, columns
    int periodic;
    int ghost;           // ghost rows on each side (0 for a whole lattice)
    int wrap_rows;       // whole periodic lattice on one GPU: vertical neighbours wrap inside the buffer
    size_t pitch;
    int8_t* alloc[2];    // ping-pong buffers (second one allocated on first tiled launch)
    int cur;
    uint64_t table[25];
    int have_table;
    int kernel, sweeps_per_launch;
    int64_t* d_obs;      // 2 x int64 accumulators
    hipEvent_t ev0, ev1;
    int timed, timing;
    unsigned long long launches;  // sweep-kernel launches so far
    uint64_t* d_xbuf;    // tile-resident kernel: exchange strips
    size_t xbuf_cap;     // bytes allocated (so are batch_cap and obs_batch_cap: ising2d_grow)
    uint32_t xgen;       // generations numbered so far in d_xbuf (every strip element carries its generation number)
    uint64_t xsig;       // strip layout the numbering belongs to (0: buffer not cleared yet)
    uint64_t xrestarts;  // times the numbering started at 1 over a cleared buffer (first use, generation limit, another strip layout)
    void* d_batch;       // tsu_ising2d_sweep_batch: device copy of the per-lattice launch items
    size_t batch_cap;
    void* d_obs_batch;   // tsu_ising2d_observables_batch: [n][2] sums of the batch (lives with its first lattice)
    size_t obs_batch_cap;
    int* h_err;          // host-mapped flag: 1 = a bounded wait of the tile-resident kernel expired, 2 = a capped union / find
                         // loop of a cluster kernel expired (results invalid either way)
    tsu_sw_scratch sw;   // K6 cluster steps: labels (1 GiB at 16384^2), batch items, launches (not counted in `launches`)
    float* d_dis;        // K7 quenched disorder: J_right, J_down, h planes of rows x pitch fp32 each (pads 0), first set_disorder
    int have_disorder;   // set_disorder called and not cleared since
    double* d_dis_part;  // K7 energy: per-workgroup partials + the total
    size_t dis_part_cap;
    unsigned long long dis_launches;  // K7 sweep-kernel launches so far (not counted in `launches`)
    long long* d_prof;   // tsu_ising2d_profiles: rows + cols int64 bins (ising2d_grow)
    size_t prof_cap;
};

// grow-only device buffer: reallocated (contents dropped) only when it holds fewer than `bytes`; no memset, no synchronisation
template <typename T>
static inline hipError_t ising2d_grow(T*& p, size_t& cap, size_t bytes) {
    if (cap >= bytes) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    const hipError_t e = hipMalloc((void**)&p, bytes);
    if (e == hipSuccess) cap = bytes;
    return e;
}

// Philox key and stream tags of a sweep (K1Params, TiledParams, PlanesItem)
template <typename P>
static inline void ising2d_set_keys(P& p, uint64_t seed, uint32_t replica) {
    p.k0 = (uint32_t)seed;
    p.k1 = (uint32_t)(seed >> 32);
    p.tag_hi = TSU_TAG_ISING_HI | (replica << 8);
    p.tag_lo = TSU_TAG_ISING_LO | (replica << 8);
}

// ising2d.hip: report (and clear) a flag a kernel left in h_err
int ising2d_check_err(tsu_ising2d* L);

// ising2d_tiled.hip
int tsu_ising2d_tiled_supported(const tsu_ising2d* L);
int tsu_ising2d_tiled_tiles(const tsu_ising2d* L);
int tsu_ising2d_tiled_sweep(tsu_ising2d* L, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica, int part);
int tsu_ising2d_tiled_part_supported(const tsu_ising2d* L);
int tsu_ising2d_planes_supported(const tsu_ising2d* L);
int tsu_ising2d_planes_sweep(tsu_ising2d* const* lats, int n, int n_sweeps, const uint64_t* seeds, const uint32_t* sweep0s,
                             const uint32_t* replicas);

// multispin_host.h -- what K9's translation units share on the host: the tsu_msc handle (multispin.hip owns it), the kernels'
// parameter block built from it, and the two entry points that cross between multispin.hip and multispin_pt.hip.  Neither of those
// is part of the C ABI: both are hidden symbols of libtsu_hip.so.
#pragma once
#include "multispin_dev.h"

struct msc_pt;  // the tempering state of a handle (multispin_pt.hip); NULL until tsu_msc_pt_enable

struct tsu_msc {
    tsu_ctx* ctx;
    MscGeo g;
    int nT, A, S, W;
    int route;
    uint64_t* d_s;       // nT * A * W planes
    uint64_t* d_j;       // 3 * W planes
    uint64_t* d_tab;     // nT * 13
    uint32_t* d_key;     // nT * A * 2
    unsigned long long* d_out;  // the measurement's counters
    int have_T, have_seeds;
    unsigned long long launches;
    msc_pt* pt;
};

namespace {

inline long long msc_bonds(const MscGeo& g) {
    const long long n = g.nsites;
    return (g.pc ? n : n / g.cols * (g.cols - 1)) + (g.pr ? n : n / g.rows * (g.rows - 1)) + (g.pz ? n : n / g.depth * (g.depth - 1));
}

inline MscParams msc_params(const tsu_msc* h) {
    MscParams p = {};
    p.g = h->g;
    p.s = h->d_s;
    p.j = h->d_j;
    p.tab = h->d_tab;
    p.key = h->d_key;
    p.A = h->A;
    p.W = h->W;
    return p;
}

inline size_t msc_planes(const tsu_msc* h) { return (size_t)h->nT * h->A * h->W; }

// entries of one measurement row: [unsat: nT A W 64][up: nT A W 64][qx: nT W 64][lx: nT W 64], the last two with two replicas
inline size_t msc_row_len(const tsu_msc* h) {
    const size_t col = (size_t)h->W * 64;
    return 2 * (size_t)h->nT * h->A * col + (h->A == 2 ? 2 * (size_t)h->nT * col : 0);
}

}  // namespace

// multispin.hip: one launch of k9_measure on the handle's stream adding into `row` (msc_row_len entries, zeroed by the caller).
// Asynchronous; returns the launch's hipError_t.
__attribute__((visibility("hidden"))) hipError_t msc_enqueue_measure(tsu_msc* h, unsigned long long* row);
// multispin_pt.hip: frees h->pt (tsu_msc_destroy calls it after the stream has drained)
__attribute__((visibility("hidden"))) void msc_pt_free(tsu_msc* h);

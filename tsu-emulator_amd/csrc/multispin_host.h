// multispin_host.h -- what K9's translation units share on the host: the tsu_msc handle (multispin.hip owns it), the kernels'
// parameter block built from it, and the entry points that cross between multispin.hip, multispin_pt.hip, multispin_corr.hip
// and multispin_quench.hip.
// None of those is part of the C ABI: all are hidden symbols of libtsu_hip.so.
#pragma once
#include "multispin_dev.h"

struct msc_pt;    // the tempering state of a handle (multispin_pt.hip); NULL until tsu_msc_pt_enable
struct msc_corr;  // the profiles' scratch and the correlation state (multispin_corr.hip); NULL until first used
struct msc_quench;  // C4 rows, snapshots and the record of a quench run (multispin_quench.hip); NULL until first used

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
    msc_corr* corr;
    msc_quench* qn;
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
// multispin.hip: n_sweeps sweeps from counter sweep0 by the handle's route on its stream, exactly tsu_msc_sweep's launches; adds
// their number to *launches.  Asynchronous; returns the launches' hipError_t.
__attribute__((visibility("hidden"))) hipError_t msc_enqueue_sweeps(tsu_msc* h, int n_sweeps, uint32_t sweep0, unsigned long long* launches);
// multispin_pt.hip: frees h->pt (tsu_msc_destroy calls it after the stream has drained)
__attribute__((visibility("hidden"))) void msc_pt_free(tsu_msc* h);
// multispin_corr.hip: frees h->corr (tsu_msc_destroy calls it after the stream has drained)
__attribute__((visibility("hidden"))) void msc_corr_free(tsu_msc* h);
// multispin_quench.hip: frees h->qn (tsu_msc_destroy calls it after the stream has drained)
__attribute__((visibility("hidden"))) void msc_quench_free(tsu_msc* h);
// multispin_corr.hip, for tsu_msc_pt_run.  msc_corr_on: tsu_msc_set_correlation switched the modes on.  Then a run calls
// msc_corr_record_begin once (a record of n_rows rows of modes replaces the last run's; 0: that run records none; returns a TSU_
// code) and, per recording round, msc_corr_enqueue_row between the round's measurement and its swap pass: kMscCorrLaunches
// launches on the handle's stream that write the modes of the planes as they are into row r.  Asynchronous.
constexpr int kMscCorrLaunches = 2;  // k9_profile, k9_modes
__attribute__((visibility("hidden"))) int msc_corr_on(const tsu_msc* h);
__attribute__((visibility("hidden"))) int msc_corr_record_begin(tsu_msc* h, int n_rows);
__attribute__((visibility("hidden"))) hipError_t msc_corr_enqueue_row(tsu_msc* h, int r);

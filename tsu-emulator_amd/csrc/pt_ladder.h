// pt_ladder.h -- what the 2-D and the 3-D parallel-tempering handles (tsu_pt2d, tsu_pt3d) have in common, as a plain struct both
// derive from: the tables, counters and history buffers of the ladders and the shape the dimension-blind kernels see (pt_dev.h,
// reduce_dev.h).  The functions on it are pt_host.h's; a unit that only reads the handle (ising2d_icm.hip) includes this alone.
#pragma once
#include "pt_dev.h"  // kPtMaxTemps

// S samples of n_ladders ladders of R walkers (whole lattices); a sample is ONE disorder.  The ladder handles have S = 1; a tempering
// ensemble (pte_host.h) has S >= 1, and every table below gains the sample as its leading index: walker g = (s * nl + k) * R + w
struct pt_ladder {
    tsu_ctx* ctx;
    const char* name;              // "pt2d" / "pt3d": the prefix of the messages
    int R, nl, nw;                 // temperatures, ladders, walkers (S * nl * R)
    int S;                         // disorder samples (the ladder handles: 1)
    int have_T, have_init;
    uint32_t sweeps, rounds;       // sweeps of every walker and rounds since init
    unsigned long long launches;   // half-sweep launches
    int hist_rounds;               // rows recorded by the last run
    size_t hist_cap;               // rows the history buffers hold
    long long nrows, pitch;        // a walker's spin plane: nrows rows (2-D: rows, 3-D: depth * rows) of pitch bytes,
    int cols;                      // the first cols of each counting
    int8_t** d_s;                  // walker g = ladder * R + w -> its spin plane
    uint32_t* d_key;               // walker -> (k0, k1)
    int32_t* d_slot;               // [ladder][walker] -> slot
    int32_t* d_was;                // [ladder][slot] -> walker
    int32_t* d_flag;               // [ladder][walker] -> round-trip flag
    double* d_T;                   // slot -> T
    float* d_c32;                  // slot -> fl32(2 / T)
    long long* d_att;              // [ladder][pair]
    long long* d_acc;
    long long* d_trips;            // [ladder][walker]
    double* d_part;                // [walker][kEnergyBlocks] energy partials
    long long* d_ipart;            // [walker][kEnergyBlocks] sum-of-spin partials
    double* d_E;                   // walker -> E of the last energy pass
    long long* d_M;                // walker -> sum of spins
    double* d_hE;                  // [round][ladder][slot]
    long long* d_hM;
    int32_t* d_hW;
    long long* d_hq;               // [round][slot] (two ladders)
    uint32_t key0, key1;           // Philox key of the swap uniforms (the seed)
    uint32_t* d_skey;              // sample -> (k0, k1) of the swap uniforms (ensembles; NULL: key0, key1)
    // correlation recording (corr_dev.h): the lattice's axes as the handle's create fills them in, then what set_correlation adds
    int n_axes, lrows;             // axes (2 or 3) and the rows of a layer (2-D: nrows)
    int axis_len[3], axis_per[3];  // length and periodic flag per axis, in axis order (2-D: rows, cols; 3-D: depth, rows, cols)
    int corr;                      // a recording round also records the k_min modes
    int hist_modes;                // the last run's rows have them
    long long* d_prof;             // [slot][sum of axis_len] profile scratch (first set_correlation / profiles call)
    double* d_tab;                 // per periodic axis, in axis order: cos[len], sin[len] (first set_correlation)
    double* d_hF;                  // [round][slot][periodic axis][re, im]
    // link overlap (link_dev.h): set_link_overlap, two ladders only
    int link;                      // a recording round also records L per slot
    int hist_link;                 // the last run's rows have it
    long long* d_hL;               // [round][slot]
    double h_T[kPtMaxTemps];       // host copy of d_T
};

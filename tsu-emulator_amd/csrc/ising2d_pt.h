// ising2d_pt.h -- the parallel-tempering handle shared by ising2d_disorder.hip (sweeps, energies, swaps) and ising2d_icm.hip
// (replica cluster moves between the two ladders).
#pragma once
#include "ising2d.h"
#include "pt_dev.h"  // kPtMaxTemps and the swap pass both ladder handles share

struct tsu_pt2d {
    tsu_ctx* ctx;
    int R, nl, nw;                 // temperatures, ladders, walkers (R * nl)
    tsu_ising2d** lat;             // walker g = ladder * R + w; lat[0] also holds the one disorder
    int have_T, have_init;
    uint32_t sweeps, rounds;       // sweeps of every walker and rounds since init
    unsigned long long launches;   // k7_pt_sweep launches
    int hist_rounds;               // rows recorded by the last run
    size_t hist_cap;               // rows the history buffers hold
    int8_t** d_s;                  // walker -> alloc[cur] of its lattice
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
    double h_T[kPtMaxTemps];       // host copy of d_T (which slots take part in the cluster moves)
    // replica cluster moves (ising2d_icm.hip); icm_every = 0: off, none of the buffers below exists
    int icm_every;                 // round t ends its sweeps with a pass iff t % icm_every == 0
    double icm_tmax;               // a slot takes part iff T[slot] <= icm_tmax
    int icm_n;                     // participating slots
    int32_t* d_icm_slots;          // their indices, ascending
    int32_t* d_icm_labels;         // tiled route: [participating slot][rows * cols] roots
    size_t icm_labels_cap;
    long long* d_icm_stats;        // [3][R]: passes, clusters, flipped sites (per walker), cumulative since init
    uint32_t icm_passes;           // the cluster-pass counter m
    unsigned long long icm_launches;
};

// ising2d_icm.hip: hooks of the tsu_pt2d_* entry points in ising2d_disorder.hip
int pt2d_icm_slots(tsu_pt2d* P);    // after set_temperatures: which slots take part (synchronises; no-op while the move is off)
int pt2d_icm_reset(tsu_pt2d* P);    // init: pass counter and statistics to 0
int pt2d_icm_enqueue(tsu_pt2d* P);  // one pass over the participating slots, asynchronous
void pt2d_icm_free(tsu_pt2d* P);

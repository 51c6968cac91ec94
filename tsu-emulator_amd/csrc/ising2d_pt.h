// ising2d_pt.h -- the 2-D parallel-tempering handle shared by ising2d_disorder.hip (sweeps, energy partials, the entry points) and
// ising2d_icm.hip (replica cluster moves between the two ladders): pt_ladder.h's ladder plus the walkers and the cluster-move state
// (h_T of the ladder says which slots take part).
#pragma once
#include "ising2d.h"
#include "pt_ladder.h"  // the tables and counters both ladder handles share

struct tsu_pt2d : pt_ladder {
    tsu_ising2d** lat;             // walker g = ladder * R + w; lat[0] also holds the one disorder (d_s[g] = alloc[cur] of lat[g])
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

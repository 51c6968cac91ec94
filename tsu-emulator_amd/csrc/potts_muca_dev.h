// potts_muca_dev.h -- K11's host-side rule: the geometry (bond count, z_max) and the acceptance table of the multicanonical Potts
// walkers (include/tsu_hip_potts_muca.h).  Plain C++, no HIP: the library and host-side checks share it.
#pragma once
#include <math.h>
#include <stdint.h>

// ctr[3] stream tag of the walkers' Philox blocks (low byte; bits 8.. carry the replica id): the value after tsu_common.h's
// TSU_TAG_SW_GHOST = 12.  DESIGN.md "RNG stream contract".
enum : uint32_t { TSU_TAG_POTTS_MUCA = 13 };

struct MucaGeom {
    int depth, rows, cols;
    int pz, pr, pc;
    int sites;
    int bonds;  // B, a periodic axis of length 2 counted twice, one of length 1 not at all
    int zmax;   // the largest |delta n| of one update
};

static inline long long muca_axis_bonds(long long sites, int len, int periodic) {
    return (sites / len) * ((len - 1) + ((periodic && len >= 2) ? 1 : 0));
}

// false for a side < 1 or more than max_sites sites
static inline bool muca_geometry(int depth, int rows, int cols, int pz, int pr, int pc, long long max_sites, MucaGeom* g) {
    if (depth < 1 || rows < 1 || cols < 1) return false;
    const long long sites = (long long)depth * rows * cols;
    if ((long long)depth * rows > max_sites || sites > max_sites) return false;
    g->depth = depth;
    g->rows = rows;
    g->cols = cols;
    g->pz = pz != 0;
    g->pr = pr != 0;
    g->pc = pc != 0;
    g->sites = (int)sites;
    g->bonds = (int)(muca_axis_bonds(sites, depth, g->pz) + muca_axis_bonds(sites, rows, g->pr) + muca_axis_bonds(sites, cols, g->pc));
    g->zmax = (depth == 1 && !g->pz) ? 4 : 6;
    return true;
}

// thr of a move from weight ln W = from to ln W = to: accepted iff (uint64)u < thr
static inline uint64_t muca_threshold(double from, double to) {
    if (to >= from) return 1ull << 32;
    return (uint64_t)floor(exp(to - from) * 4294967296.0);
}

// out[n (2 zmax + 1) + delta + zmax], 0 where n + delta lies outside 0 .. bonds
static inline void muca_thresholds(long long bonds, int zmax, const double* lnw, uint64_t* out) {
    const int K = 2 * zmax + 1;
    for (long long n = 0; n <= bonds; ++n)
        for (int d = -zmax; d <= zmax; ++d) {
            const long long to = n + d;
            out[n * K + d + zmax] = (to < 0 || to > bonds) ? 0ull : muca_threshold(lnw[n], lnw[to]);
        }
}

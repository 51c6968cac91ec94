// pt_dev.h -- the swap pass of parallel tempering, shared by the 2-D ladders (tsu_pt2d, ising2d_disorder.hip) and the 3-D ladders
// (tsu_pt3d, ising3d.hip).  The pass sees walkers, slots and energies only: it does not know the lattice's dimension, so both
// handle types launch this one kernel ("Parallel tempering (K7)").  Everything here has internal linkage:
// each translation unit that includes the header gets its own copy of the kernel.
#pragma once
#include "dense.h"
#include "tsu_common.h"

constexpr int kPtMaxTemps = 256;

namespace {

enum : int { kPtNone = 0, kPtBottom = 1, kPtTop = 2 };  // round-trip flag of a walker

struct PTSwap {
    const double* E;     // walker -> energy of this round
    const long long* M;  // walker -> sum of spins
    const double* T;     // slot -> T
    int32_t* was;        // [ladder][slot] -> walker
    int32_t* slot;       // [ladder][walker] -> slot
    int32_t* flag;       // [ladder][walker] -> kPtNone / kPtBottom / kPtTop
    long long* att;      // [ladder][pair] attempts, accepts
    long long* acc;
    long long* trips;    // [ladder][walker] round trips
    double* hE;          // this round's history row [ladder][slot] (NULL: not recorded)
    long long* hM;
    int32_t* hW;
    int R, do_swap;
    uint32_t t, k0, k1;  // round counter; Philox key = seed
};

__device__ __forceinline__ void pt_arrive(int* flag, long long* trips, int w, int slot, int R) {
    if (slot == 0) {
        if (flag[w] == kPtTop) trips[w] += 1;
        flag[w] = kPtBottom;
    } else if (slot == R - 1 && flag[w] == kPtBottom) {
        flag[w] = kPtTop;
    }
}

// one wave per ladder: the pairs' uniforms in parallel, the pass in the reference's order (gibbs.py:309-323) by lane 0, then the
// tables and the history row.  Swap (a at slot i, b at slot i + 1) with probability min(1, exp((1/T_i - 1/T_{i+1}) (E_a - E_b))),
// the ratio of the Boltzmann weights after and before: detailed balance for the product measure of the ladder.
__global__ __launch_bounds__(64) void k7_pt_swap(PTSwap p) {
    const int k = blockIdx.x, R = p.R;
    __shared__ double u[kPtMaxTemps], e[kPtMaxTemps];
    __shared__ int was[kPtMaxTemps], flag[kPtMaxTemps];
    for (int i = threadIdx.x; i < R; i += 64) {
        was[i] = p.was[k * R + i];
        flag[i] = p.flag[k * R + i];
        e[i] = p.E[k * R + i];
        if (p.do_swap && i + 1 < R) u[i] = dense_uniform((uint32_t)i, p.t, TSU_TAG_PT_SWAP | ((uint32_t)k << 8), p.k0, p.k1);
    }
    __syncthreads();
    if (threadIdx.x == 0 && p.do_swap) {
        long long* att = p.att + k * (R - 1);
        long long* acc = p.acc + k * (R - 1);
        long long* trips = p.trips + k * R;
        for (int i = 0; i + 1 < R; ++i) {
            const int a = was[i], b = was[i + 1];
            // the reference's expression with E_a - E_b: its E_b - E_a (gibbs.py:317) inverts the detailed-balance ratio
            const double delta = (1.0 / p.T[i] - 1.0 / p.T[i + 1]) * (e[a] - e[b]);
            att[i] += 1;
            if (delta >= 0.0 || u[i] < exp(delta)) {
                acc[i] += 1;
                was[i] = b;
                was[i + 1] = a;
                pt_arrive(flag, trips, a, i + 1, R);
                pt_arrive(flag, trips, b, i, R);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < R; i += 64) {
        const int w = was[i];
        p.was[k * R + i] = w;
        p.slot[k * R + w] = i;
        p.flag[k * R + i] = flag[i];
        if (p.hE) {
            p.hE[k * R + i] = e[w];
            p.hM[k * R + i] = p.M[k * R + w];
            p.hW[k * R + i] = w;
        }
    }
}

}  // namespace

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
    int nl;              // ladders per sample: workgroup b is ladder b % nl of sample b / nl (a ladder handle: one sample)
    const uint32_t* skey;  // sample -> (k0, k1) (NULL: k0, k1 above, one sample)
};

__device__ __forceinline__ void pt_arrive(int* flag, long long* trips, int w, int slot, int R) {
    if (slot == 0) {
        if (flag[w] == kPtTop) trips[w] += 1;
        flag[w] = kPtBottom;
    } else if (slot == R - 1 && flag[w] == kPtBottom) {
        flag[w] = kPtTop;
    }
}

// one wave per ladder (of every sample: the tables are [sample][ladder][..], so workgroup b finds its rows at b R): the pairs' uniforms in parallel, the pass in the reference's order (gibbs.py:309-323) by lane 0, then the
// tables and the history row.  Swap (a at slot i, b at slot i + 1) with probability min(1, exp((1/T_i - 1/T_{i+1}) (E_a - E_b))),
// the ratio of the Boltzmann weights after and before: detailed balance for the product measure of the ladder.
__global__ __launch_bounds__(64) void k7_pt_swap(PTSwap p) {
    const int k = blockIdx.x, R = p.R;  // k: the row of the tables, (sample, ladder)
    const int smp = k / p.nl;
    const uint32_t lad = (uint32_t)(k - smp * p.nl);
    const uint32_t k0 = p.skey ? p.skey[2 * smp] : p.k0, k1 = p.skey ? p.skey[2 * smp + 1] : p.k1;
    __shared__ double u[kPtMaxTemps], e[kPtMaxTemps];
    __shared__ int was[kPtMaxTemps], flag[kPtMaxTemps];
    for (int i = threadIdx.x; i < R; i += 64) {
        was[i] = p.was[k * R + i];
        flag[i] = p.flag[k * R + i];
        e[i] = p.E[k * R + i];
        if (p.do_swap && i + 1 < R) u[i] = dense_uniform((uint32_t)i, p.t, TSU_TAG_PT_SWAP | (lad << 8), k0, k1);
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

// ---------------------------------------------------------------- all walkers of an ensemble in one launch (pte_host.h)
// i.i.d. +-1 for every walker: walker y gets the bits of tsu_ising2d_randomize / tsu_ising3d_randomize with its own key key[y] and
// replica 0 (Philox(q >> 3, rho, 0, TAG_INIT); pad bytes 0), as pop_randomize does for seed + y.  grid (ceil(nrows nchunks / 256), nw)
__global__ __launch_bounds__(256) void pt_randomize_all(int8_t* const* __restrict__ s, const uint32_t* __restrict__ key, long long nrows,
                                                        long long pitch, int cols) {
    const int nchunks = (cols + 15) >> 4;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nrows * nchunks) return;
    const long long rho = t / nchunks;
    const int q = (int)(t - rho * nchunks);
    const u32x4 w = tsu_philox((uint32_t)(q >> 3), (uint32_t)rho, 0u, TSU_TAG_INIT, key[2 * blockIdx.y], key[2 * blockIdx.y + 1]);
    const uint32_t wv[4] = {w.x, w.y, w.z, w.w};
    const uint32_t bits = (wv[(q & 7) >> 1] >> (16 * (q & 1))) & 0xFFFFu;
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = 4 * k + b;
            uint32_t byte = ((bits >> i) & 1u) ? 0x01u : 0xFFu;
            if (16 * q + i >= cols) byte = 0;
            v |= byte << (8 * b);
        }
        o[k] = v;
    }
    *reinterpret_cast<uint4*>(s[blockIdx.y] + rho * pitch + 16 * q) = make_uint4(o[0], o[1], o[2], o[3]);
}

// every spin of every walker = value (+1 / -1), pad bytes 0; the same grid
__global__ __launch_bounds__(256) void pt_fill_all(int8_t* const* __restrict__ s, int value, long long nrows, long long pitch, int cols) {
    const int nchunks = (cols + 15) >> 4;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nrows * nchunks) return;
    const long long rho = t / nchunks;
    const int q = (int)(t - rho * nchunks);
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t byte = (16 * q + 4 * k + b < cols) ? (uint32_t)(uint8_t)value : 0u;
            v |= byte << (8 * b);
        }
        o[k] = v;
    }
    *reinterpret_cast<uint4*>(s[blockIdx.y] + rho * pitch + 16 * q) = make_uint4(o[0], o[1], o[2], o[3]);
}

}  // namespace

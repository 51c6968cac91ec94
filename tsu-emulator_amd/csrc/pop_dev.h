// pop_dev.h -- the resampling step of population annealing, shared by the 2-D populations (tsu_pa2d, ising2d_disorder.hip) and the
// 3-D populations (tsu_pa3d, ising3d.hip).  Nothing here knows the lattice's dimension: a walker's spin plane is `nrows` rows of
// `pitch` bytes (pitch a multiple of 16), the sweeps and the energy pass stay with their dimension (k7_pt_sweep / k8_pt_sweep,
// k7_pt_energy / k8_pt_energy, unchanged).  DESIGN.md section 3, "Population annealing".  Everything here has internal linkage:
// each translation unit that includes the header gets its own copy of the kernels.
//
// One step from beta to beta + db, population of R walkers with energies E_i (float64, the energy pass's bits):
//   E_min = min_i E_i;  w_i = exp(-(db (E_i - E_min))) in float64;  W_i = (uint32) rint(w_i 2^30);  S = sum_i W_i (an integer).
//   U = mulhi64(x64, S), x64 = (w1 << 32) | w0 of Philox(0, 0, k_abs, TAG_POP_RESAMPLE), key = seed.
//   n_i = (R C_i + U) / S - (R C_{i-1} + U) / S with the inclusive prefix sums C_i of W (C_{-1} = 0), integer division: systematic
//   resampling at fixed size, sum_i n_i = R exactly, n_i = floor or ceil of R W_i / S.  R C_i + U < 2^16 2^46 + 2^46 < 2^63.
//   A walker with n_i >= 1 stays (parent[i] = i); the dead indices in ascending order take the extra copies in ascending order of
//   their source (source g: n_g - 1 times).  pop_copy then copies plane parent[i] -> i for the dead i: sources are survivors and
//   are never written, destinations are dead and are never read.
#pragma once
#include "tsu_common.h"

constexpr int kPopMaxWalkers = 65535;  // grid.y of the energy pass, and R C_i < 2^62
constexpr int kPopPlanThreads = 1024;

namespace {

struct PopPlan {
    const double* E;        // walker -> energy of the last pass
    uint32_t* W;            // walker -> 30-bit weight (a history row or scratch)
    int32_t* parent;        // walker -> the walker whose plane it holds after the copy (a history row or scratch)
    uint32_t* xs;           // [R + 1] scratch: exclusive prefix of the extra copies, xs[i] = sum_{g < i} max(n_g - 1, 0)
    int32_t* dead;          // [R] scratch: the dead indices, ascending
    int2* pairs;            // [R] (dst, src) of the copies
    uint32_t* n_pairs;      // their number
    unsigned long long* S;  // this step's record (NULL: not recorded)
    unsigned long long* U;
    double* Emin;
    double db;
    int R;
    uint32_t k_abs, k0, k1;  // step counter; Philox key = seed
};

// exclusive scan of v over the workgroup's 1024 threads (thread order), total to everyone; wtot: 16 words of LDS, free again on return
__device__ __forceinline__ unsigned long long pop_scan(unsigned long long v, unsigned long long* wtot, unsigned long long& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long x = v;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    if (lane == 63) wtot[wave] = x;
    __syncthreads();
    unsigned long long base = 0, tot = 0;
    for (int w = 0; w < kPopPlanThreads / 64; ++w) {
        if (w < wave) base += wtot[w];
        tot += wtot[w];
    }
    __syncthreads();
    total = tot;
    return base + x - v;
}

// One workgroup: weights, the resampling counts and the placement of a step, for any R <= kPopMaxWalkers.  Thread t owns the
// contiguous chunk [t c, t c + c) of walkers, c = ceil(R / 1024); chunk totals are scanned in LDS and the chunk's values are read
// again from global memory, so LDS does not grow with R.
__global__ __launch_bounds__(kPopPlanThreads) void pop_plan(PopPlan p) {
    __shared__ unsigned long long wtot[kPopPlanThreads / 64];
    __shared__ double wmin[kPopPlanThreads / 64];
    const int R = p.R, t = threadIdx.x;
    const int c = (R + kPopPlanThreads - 1) / kPopPlanThreads;
    const int lo = min(t * c, R), hi = min(lo + c, R);

    // E_min: a minimum does not depend on the order
    double m = INFINITY;
    for (int i = lo; i < hi; ++i) m = fmin(m, p.E[i]);
    for (int off = 32; off > 0; off >>= 1) m = fmin(m, __shfl_xor(m, off, 64));
    if ((t & 63) == 0) wmin[t >> 6] = m;
    __syncthreads();
    double emin = wmin[0];
    for (int w = 1; w < kPopPlanThreads / 64; ++w) emin = fmin(emin, wmin[w]);

    // weights and their sum: integers from here on
    unsigned long long sum = 0;
    for (int i = lo; i < hi; ++i) {
        const double d = p.E[i] - emin;
        const double x = p.db * d;
        const uint32_t W = (uint32_t)rint(exp(-x) * 1073741824.0);
        p.W[i] = W;
        sum += W;
    }
    unsigned long long S;
    const unsigned long long C = pop_scan(sum, wtot, S);  // sum of W before this chunk
    if (S == 0) {  // only if no energy is a number (the minimum's weight is 2^30 otherwise): nobody moves
        for (int i = lo; i < hi; ++i) p.parent[i] = i;
        if (t == 0) {
            *p.n_pairs = 0;
            if (p.S) {
                *p.S = 0;
                *p.U = 0;
                *p.Emin = emin;
            }
        }
        return;
    }

    const u32x4 ph = tsu_philox(0u, 0u, p.k_abs, TSU_TAG_POP_RESAMPLE, p.k0, p.k1);
    const unsigned long long x64 = ((unsigned long long)ph.y << 32) | ph.x;
    const unsigned long long U = __umul64hi(x64, S);
    if (t == 0 && p.S) {
        *p.S = S;
        *p.U = U;
        *p.Emin = emin;
    }

    // counts: the chunk's dead walkers and extra copies (each <= 65535: both fit one 64-bit scan, dead in the high half)
    uint32_t nd = 0, nx = 0;
    {
        unsigned long long Ci = C, before = ((unsigned long long)R * C + U) / S;
        for (int i = lo; i < hi; ++i) {
            Ci += p.W[i];
            const unsigned long long upto = ((unsigned long long)R * Ci + U) / S;
            const uint32_t n = (uint32_t)(upto - before);
            before = upto;
            nd += n == 0 ? 1u : 0u;
            nx += n > 1 ? n - 1 : 0u;
        }
    }
    unsigned long long tot2;
    const unsigned long long off2 = pop_scan(((unsigned long long)nd << 32) | nx, wtot, tot2);
    uint32_t doff = (uint32_t)(off2 >> 32), xoff = (uint32_t)off2;
    const uint32_t n_dead = (uint32_t)(tot2 >> 32);  // == the number of extra copies, since sum n = R
    {
        unsigned long long Ci = C, before = ((unsigned long long)R * C + U) / S;
        for (int i = lo; i < hi; ++i) {
            Ci += p.W[i];
            const unsigned long long upto = ((unsigned long long)R * Ci + U) / S;
            const uint32_t n = (uint32_t)(upto - before);
            before = upto;
            p.xs[i] = xoff;
            xoff += n > 1 ? n - 1 : 0u;
            if (n == 0) p.dead[doff++] = i;
            else p.parent[i] = i;
        }
    }
    if (t == kPopPlanThreads - 1) p.xs[R] = (uint32_t)tot2;
    if (t == 0) *p.n_pairs = n_dead;
    __syncthreads();  // xs and dead are complete (global writes of this workgroup)

    // dead walker number j takes extra copy number j: its source is the last g with xs[g] <= j (then xs[g + 1] > j: g has extras)
    for (uint32_t j = t; j < n_dead; j += kPopPlanThreads) {
        int a = 0, b = R;  // xs[a] <= j < xs[b]
        while (b - a > 1) {
            const int mid = (a + b) >> 1;
            if (p.xs[mid] <= j) a = mid;
            else b = mid;
        }
        const int dst = p.dead[j];
        p.parent[dst] = a;
        p.pairs[j] = make_int2(dst, a);
    }
}

// parent rows of a run that does not resample: the identity
__global__ __launch_bounds__(256) void pop_identity(int32_t* __restrict__ parent, int R, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) parent[i] = (int32_t)(i % R);
}

// Planes pairs[j].y -> pairs[j].x for j < *n_pairs, a plane = cpp chunks of 16 bytes.  A fixed flat grid strides over the
// (pair, tile of 256 chunks) items; the count is read from the device, so the host never waits for the plan.  A workgroup with
// nothing to do exits.
__global__ __launch_bounds__(256) void pop_copy(int8_t* const* __restrict__ s, const int2* __restrict__ pairs,
                                                const uint32_t* __restrict__ n_pairs, uint32_t cpp) {
    const uint32_t tpp = (cpp + 255u) / 256u;
    const unsigned long long items = (unsigned long long)*n_pairs * tpp;
    for (unsigned long long it = blockIdx.x; it < items; it += gridDim.x) {
        const uint32_t j = (uint32_t)(it / tpp);
        const uint32_t ch = (uint32_t)(it - (unsigned long long)j * tpp) * 256u + threadIdx.x;
        if (ch >= cpp) continue;
        const int2 pr = pairs[j];
        const uint4* __restrict__ src = reinterpret_cast<const uint4*>(s[pr.y]);
        uint4* __restrict__ dst = reinterpret_cast<uint4*>(s[pr.x]);
        dst[ch] = src[ch];
    }
}

// i.i.d. +-1 for every walker: walker y gets the bits of tsu_ising2d_randomize(seed + y, 0) / tsu_ising3d_randomize(seed + y, 0)
// (Philox(q >> 3, rho, 0, TAG_INIT), key = seed + y; pad bytes 0).  grid (ceil(nrows nchunks / 256), R)
__global__ __launch_bounds__(256) void pop_randomize(int8_t* const* __restrict__ s, unsigned long long seed, long long nrows,
                                                     long long pitch, int cols) {
    const int nchunks = (cols + 15) >> 4;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nrows * nchunks) return;
    const long long rho = t / nchunks;
    const int q = (int)(t - rho * nchunks);
    const unsigned long long key = seed + blockIdx.y;
    const u32x4 w = tsu_philox((uint32_t)(q >> 3), (uint32_t)rho, 0u, TSU_TAG_INIT, (uint32_t)key, (uint32_t)(key >> 32));
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

}  // namespace

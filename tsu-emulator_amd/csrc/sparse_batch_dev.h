// sparse_batch_dev.h -- the kernels of a walker batch on one sparse graph (tsu_sparse_batch, sparse_batch.hip; DESIGN.md section 5,
// "K5 walker batches").  Internal linkage throughout.
//
// State layout (private to the handle): state[position][walker], one byte {0,1} each, WP = walkers padded to a multiple of 16 bytes
// per position, pad bytes 0.  A thread of the colour route owns ONE position and a chunk of W consecutive walkers (W = 4, 8, 16): it
// reads its row's col / val once and each neighbour's chunk as one dword / qword / dwordx4 (the sector a gathered byte costs anyway
// carries the other walkers), keeps W double fields, and stores its W new bytes in one instruction.  Consecutive lanes take
// consecutive chunks of one position, then the next position: a wave's row loads are near-uniform and its stores contiguous.
#pragma once
#include "dense.h"
#include "pt_dev.h"  // the swap pass k7_pt_swap, kPtMaxTemps, the round-trip flags
#include "sparse_host.h"

constexpr int K5B_PAD = 16;          // walkers per position are padded to a multiple of this many bytes
constexpr int K5B_LANES = 1024;      // strided partials of the fixed-order energy
constexpr int K5B_SEGMENT = 65536;   // positions per energy segment (64 per partial); n <= 65536: one segment
constexpr int K5B_THREADS = 1024;    // workgroup of the energy pass and of the small route

namespace {

template <int W>
struct alignas(W) K5BChunk {
    uint8_t b[W];
};

// what every pass over the graph is given
struct K5BArgs {
    const int64_t* row_ptr;  // position-space CSR of the graph (borrowed from the tsu_sparse handle)
    const int32_t* col;
    const double* val;
    const double* bias;
    const int32_t* site_of;
    int8_t* state;           // [n][WP]
    const int32_t* slot;     // walker -> slot
    const double* T;         // slot -> T
    int n, nw, WP;
    uint32_t k0, k1;
};

// the fields of W walkers of row p: F_k = sum over the row's edges in CSR order of val * bit_k (the generic K5 expression per walker)
template <int W>
static __device__ __forceinline__ void k5b_fields(const K5BArgs& A, int p, int g0, double (&F)[W]) {
#pragma unroll
    for (int k = 0; k < W; ++k) F[k] = 0.0;
    const int64_t e0 = A.row_ptr[p], e1 = A.row_ptr[p + 1];
    for (int64_t e = e0; e < e1; ++e) {
        const double v = A.val[e];
        const K5BChunk<W> c = *reinterpret_cast<const K5BChunk<W>*>(A.state + (size_t)A.col[e] * A.WP + g0);
#pragma unroll
        for (int k = 0; k < W; ++k) F[k] += v * (double)c.b[k];
    }
}

// One colour class [pb, pe) for all walkers: thread t = (position, chunk), chunk-minor.
template <int W>
__global__ __launch_bounds__(256) void k5b_color(K5BArgs A, int pb, int pe, uint32_t sweep) {
    const int chunks = (A.nw + W - 1) / W;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)(pe - pb) * chunks) return;
    const int p = pb + (int)(t / chunks);
    const int g0 = (int)(t % chunks) * W;
    double F[W];
    k5b_fields<W>(A, p, g0, F);
    const double bias = A.bias[p];
    const uint32_t site = (uint32_t)A.site_of[p];
    K5BChunk<W> out;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const int g = g0 + k;
        uint8_t bit = 0;
        if (g < A.nw) {
            const double T = A.T[A.slot[g]];
            const double u = dense_uniform(site, sweep, TSU_TAG_DENSE | ((uint32_t)g << 8), A.k0, A.k1);
            bit = (u < sigmoid_clamped((F[k] + bias) / T)) ? 1 : 0;
        }
        out.b[k] = bit;
    }
    *reinterpret_cast<K5BChunk<W>*>(A.state + (size_t)p * A.WP + g0) = out;
}

// the halving tree over the workgroup's 1024 values: red[j] += red[j + s], s = 512 .. 1 (the caller has filled red and synchronised)
static __device__ __forceinline__ void k5b_tree(double* red, long long* redm, int j) {
    for (int s = K5B_LANES / 2; s > 0; s >>= 1) {
        if (j < s) {
            red[j] += red[j + s];
            redm[j] += redm[j + s];
        }
        __syncthreads();
    }
}

// Energy partial pass of the colour route: workgroup (segment, chunk); thread j sums the terms of the positions p = j mod 1024 of its
// segment in ascending order for its W walkers, then one tree per walker.  part / mpart: [segment][WP].
template <int W>
__global__ __launch_bounds__(K5B_THREADS) void k5b_energy(K5BArgs A, double* __restrict__ part, long long* __restrict__ mpart) {
    __shared__ double red[K5B_LANES];
    __shared__ long long redm[K5B_LANES];
    const int seg = blockIdx.x, g0 = (int)blockIdx.y * W, j = threadIdx.x;
    const int p_end = min(A.n, (seg + 1) * K5B_SEGMENT);
    double acc[W];
    int m[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        acc[k] = 0.0;
        m[k] = 0;
    }
    for (int p = seg * K5B_SEGMENT + j; p < p_end; p += K5B_LANES) {
        double F[W];
        k5b_fields<W>(A, p, g0, F);
        const double bias = A.bias[p];
        const K5BChunk<W> c = *reinterpret_cast<const K5BChunk<W>*>(A.state + (size_t)p * A.WP + g0);
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const double b = (double)c.b[k];
            acc[k] += -0.5 * b * F[k] - bias * b;
            m[k] += 2 * (int)c.b[k] - 1;
        }
    }
#pragma unroll
    for (int k = 0; k < W; ++k) {
        red[j] = acc[k];
        redm[j] = m[k];
        __syncthreads();
        k5b_tree(red, redm, j);
        if (j == 0 && g0 + k < A.nw) {
            part[(size_t)seg * A.WP + g0 + k] = red[0];
            mpart[(size_t)seg * A.WP + g0 + k] = redm[0];
        }
        __syncthreads();
    }
}

// the segments' sums in ascending order
__global__ __launch_bounds__(256) void k5b_energy_final(const double* __restrict__ part, const long long* __restrict__ mpart, int nseg, int nw,
                                                        int WP, double* __restrict__ E, long long* __restrict__ M) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= nw) return;
    double e = 0.0;
    long long m = 0;
    for (int s = 0; s < nseg; ++s) {
        e += part[(size_t)s * WP + g];
        m += mpart[(size_t)s * WP + g];
    }
    E[g] = e;
    M[g] = m;
}

// Small route (n <= K5S_MAX): workgroup g is walker g, its state in LDS; n_sweeps sweeps colour after colour with a workgroup barrier
// in between (k5_small's loop at the walker's temperature and replica), then the walker's fixed-order energy (one segment) and its
// sum of spins, then the state goes back.
__global__ __launch_bounds__(K5B_THREADS) void k5b_small(K5BArgs A, const int* __restrict__ color_off, int n_colors, int n_sweeps, uint32_t sweep0,
                                                        double* __restrict__ E, long long* __restrict__ M) {
    extern __shared__ int8_t s_state[];
    __shared__ double red[K5B_LANES];
    __shared__ long long redm[K5B_LANES];
    const int g = blockIdx.x, j = threadIdx.x, n = A.n;
    for (int p = j; p < n; p += K5B_THREADS) s_state[p] = A.state[(size_t)p * A.WP + g];
    const double T = A.T[A.slot[g]];
    const uint32_t tag = TSU_TAG_DENSE | ((uint32_t)g << 8);
    __syncthreads();
    for (int s = 0; s < n_sweeps; ++s) {
        for (int c = 0; c < n_colors; ++c) {
            const int pb = color_off[c], pe = color_off[c + 1];
            for (int p = pb + j; p < pe; p += K5B_THREADS) {
                const int64_t e0 = A.row_ptr[p], e1 = A.row_ptr[p + 1];
                double F = 0.0;
                for (int64_t e = e0; e < e1; ++e) F += A.val[e] * (double)s_state[A.col[e]];
                F += A.bias[p];
                const double u = dense_uniform((uint32_t)A.site_of[p], sweep0 + (uint32_t)s, tag, A.k0, A.k1);
                s_state[p] = (u < sigmoid_clamped(F / T)) ? 1 : 0;
            }
            __syncthreads();
        }
    }
    double acc = 0.0;
    int m = 0;
    for (int p = j; p < n; p += K5B_LANES) {
        const int64_t e0 = A.row_ptr[p], e1 = A.row_ptr[p + 1];
        double F = 0.0;
        for (int64_t e = e0; e < e1; ++e) F += A.val[e] * (double)s_state[A.col[e]];
        const double b = (double)s_state[p];
        acc += -0.5 * b * F - A.bias[p] * b;
        m += 2 * (int)s_state[p] - 1;
    }
    red[j] = acc;
    redm[j] = m;
    __syncthreads();
    k5b_tree(red, redm, j);
    if (j == 0) {
        E[g] = red[0];
        M[g] = redm[0];
    }
    for (int p = j; p < n; p += K5B_THREADS) A.state[(size_t)p * A.WP + g] = s_state[p];
}

// the start of every walker: initial 0: bit of site i of walker g = [uniform53(i, 0, TAG_INIT | g << 8, seed) < 0.5]; 1 / -1: all ones
// / all zeros.  Thread = (position, group of 4 walkers); pad bytes 0.
__global__ __launch_bounds__(256) void k5b_init(int8_t* __restrict__ state, const int32_t* __restrict__ site_of, int n, int nw, int WP, int initial,
                                                uint32_t k0, uint32_t k1) {
    const int quads = WP / 4;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)n * quads) return;
    const int p = (int)(t / quads), g0 = (int)(t % quads) * 4;
    const uint32_t site = (uint32_t)site_of[p];
    K5BChunk<4> out;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int g = g0 + k;
        uint8_t bit = 0;
        if (g < nw) {
            if (initial == 0) bit = dense_uniform(site, 0u, TSU_TAG_INIT | ((uint32_t)g << 8), k0, k1) < 0.5 ? 1 : 0;
            else bit = initial > 0 ? 1 : 0;
        }
        out.b[k] = bit;
    }
    *reinterpret_cast<K5BChunk<4>*>(state + (size_t)p * WP + g0) = out;
}

// every walker at its own slot, the walker at slot 0 "bottom", no attempts, accepts or round trips
__global__ __launch_bounds__(256) void k5b_reset(int32_t* __restrict__ slot, int32_t* __restrict__ was, int32_t* __restrict__ flag,
                                                 long long* __restrict__ att, long long* __restrict__ acc, long long* __restrict__ trips, int R,
                                                 int nw) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= nw) return;
    const int w = g % R, k = g / R;
    slot[g] = w;
    was[g] = w;
    flag[g] = w == 0 ? kPtBottom : kPtNone;
    trips[g] = 0;
    if (w + 1 < R) {
        att[k * (R - 1) + w] = 0;
        acc[k * (R - 1) + w] = 0;
    }
}

__global__ __launch_bounds__(256) void k5b_fill(double* __restrict__ x, double v, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) x[i] = v;
}

// the temperature table travels as a kernel argument: set_temperatures is enqueued like every launch and waits for nothing
struct K5BTemps {
    double T[kPtMaxTemps];
};
__global__ __launch_bounds__(256) void k5b_set_temps(K5BTemps t, int R, double* __restrict__ T) {
    const int i = threadIdx.x;
    if (i < R) T[i] = t.T[i];
}

// site-order plane <-> one walker's column of a [n][WP] array
__global__ __launch_bounds__(256) void k5b_scatter(const int8_t* __restrict__ src_site, const int32_t* __restrict__ site_of, int8_t* __restrict__ dst,
                                                   int n, int WP, int g) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < n) dst[(size_t)p * WP + g] = src_site[site_of[p]];
}

__global__ __launch_bounds__(256) void k5b_gather(const int8_t* __restrict__ src, const int32_t* __restrict__ site_of, int8_t* __restrict__ dst_site,
                                                  int n, int WP, int g) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < n) dst_site[site_of[p]] = src[(size_t)p * WP + g];
}

// best states: the masked copy (walkers whose energy of this pass is below their best so far), then the min update
__global__ __launch_bounds__(256) void k5b_best_copy(const int8_t* __restrict__ state, int8_t* __restrict__ best, const double* __restrict__ E,
                                                     const double* __restrict__ bestE, int n, int nw, int WP) {
    const int quads = WP / 4;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)n * quads) return;
    const int g0 = (int)(t % quads) * 4;
    if (g0 >= nw) return;
    const size_t at = (size_t)(t / quads) * WP + g0;
    const K5BChunk<4> s = *reinterpret_cast<const K5BChunk<4>*>(state + at);
    K5BChunk<4> b = *reinterpret_cast<const K5BChunk<4>*>(best + at);
    bool any = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int g = g0 + k;
        const bool take = g < nw && E[g] < bestE[g];
        b.b[k] = take ? s.b[k] : b.b[k];
        any = any || take;
    }
    if (any) *reinterpret_cast<K5BChunk<4>*>(best + at) = b;
}

__global__ __launch_bounds__(256) void k5b_best_min(const double* __restrict__ E, double* __restrict__ bestE, int nw) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g < nw && E[g] < bestE[g]) bestE[g] = E[g];
}

}  // namespace

// reduce_dev.h -- the reductions the disordered lattices share: K7 (ising2d_disorder.hip, 2-D) and K8 (ising3d.hip, 3-D), single
// lattices and tempering ladders alike.  Nothing here knows the lattice's dimension: a spin plane is `nrows` rows of `pitch` bytes
// (nrows = rows in 2-D, depth * rows in 3-D) of which the first `cols` count.  What reads the disorder layout (the energy lane,
// the octet) is disorder_dev.h's.  Everything here has internal linkage: each translation unit that includes the header
// gets its own copy of the kernels.
#pragma once
#include "disorder_dev.h"

namespace {

constexpr int kEnergyBlocks = 1024;  // fixed partial count: the summation order depends on the shape only

// workgroup sum of 256 lanes: fixed shuffle tree, then the four waves in a fixed order (every thread gets it).  Each of these two
// helpers owns one __shared__ array and ends without a barrier: a kernel may call each of them once (a second call would write
// wpart while slower threads still read the first result).
__device__ __forceinline__ double block_sum(double e) {
    for (int off = 32; off > 0; off >>= 1) e += __shfl_down(e, off, 64);
    __shared__ double wpart[4];
    if ((threadIdx.x & 63) == 0) wpart[threadIdx.x >> 6] = e;
    __syncthreads();
    return (wpart[0] + wpart[1]) + (wpart[2] + wpart[3]);
}

__device__ __forceinline__ long long block_isum(long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __shared__ long long wpart[4];
    if ((threadIdx.x & 63) == 0) wpart[threadIdx.x >> 6] = v;
    __syncthreads();
    return wpart[0] + wpart[1] + wpart[2] + wpart[3];
}

// -(sum of the n partials), in a fixed order (every thread gets it)
__device__ __forceinline__ double final_sum(const double* __restrict__ part, int n) {
    double e = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) e += part[i];
    return -block_sum(e);
}

// one workgroup: out[0] = E of a single lattice's n partials
__global__ __launch_bounds__(256) void energy_final(const double* __restrict__ part, int n, double* __restrict__ out) {
    const double e = final_sum(part, n);
    if (threadIdx.x == 0) out[0] = e;
}

// one workgroup per walker: E as energy_final sums it, and the sum of spins
__global__ __launch_bounds__(256) void pt_energy_final(const double* __restrict__ part, const long long* __restrict__ ipart, int n,
                                                       double* __restrict__ E, long long* __restrict__ M) {
    const size_t base = (size_t)blockIdx.x * kEnergyBlocks;
    const double e = final_sum(part + base, n);
    long long m = 0;
    for (int i = threadIdx.x; i < n; i += 256) m += ipart[base + i];
    const long long ms = block_isum(m);
    if (threadIdx.x == 0) {
        E[blockIdx.x] = e;
        M[blockIdx.x] = ms;
    }
}

// the tail of the ladders' energy kernels, grid (blocks, walkers): workgroup x's partial of walker y's energy and sum of spins from
// the lanes' shares
__device__ __forceinline__ void pt_energy_partials(double e_lane, long long m_lane, double* __restrict__ part, long long* __restrict__ ipart) {
    const double e = block_sum(e_lane);
    const long long ms = block_isum(m_lane);
    if (threadIdx.x == 0) {
        part[(size_t)blockIdx.y * kEnergyBlocks + blockIdx.x] = e;
        ipart[(size_t)blockIdx.y * kEnergyBlocks + blockIdx.x] = ms;
    }
}

// a lane's share of sum over sites of s^a s^b (b == nullptr: of s^a), columns < cols only; lane = chunk (row, q), grid-stride
// over blockIdx.x
__device__ __forceinline__ long long pair_lane(const int8_t* __restrict__ a, const int8_t* __restrict__ b, long long pitch_a,
                                               long long pitch_b, long long nrows, int cols) {
    const int nchunks = (cols + 15) >> 4;
    const long long total = nrows * nchunks;
    long long sum = 0;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long rho = t / nchunks;
        const int q = (int)(t - rho * nchunks);
        const uint4 va = *reinterpret_cast<const uint4*>(a + rho * pitch_a + 16 * q);
        int cs = 0;
        if (b) {
            const uint4 vb = *reinterpret_cast<const uint4*>(b + rho * pitch_b + 16 * q);
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (16 * q + i < cols) cs += sbyte(va, i) * sbyte(vb, i);
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (16 * q + i < cols) cs += sbyte(va, i);
        }
        sum += cs;
    }
    return sum;
}

// grid (blocks, S R): q of the two ladders' walkers of sample y / R at slot y % R, added into out[y] (a zeroed history row
// [sample][slot]); the tables are [sample][ladder][..] (a ladder handle and a population's pairs: one sample)
__global__ __launch_bounds__(256) void pt_overlap(int8_t* const* __restrict__ s, const int32_t* __restrict__ was, int R,
                                                  long long pitch, long long nrows, int cols, long long* __restrict__ out) {
    const int y = blockIdx.y, smp = y / R, i = y - smp * R;
    s += (size_t)smp * 2 * R;
    was += (size_t)smp * 2 * R;
    const long long v = block_isum(pair_lane(s[was[i]], s[R + was[R + i]], pitch, pitch, nrows, cols));
    if (threadIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long*>(out + y), (unsigned long long)v);
}

// workgroups of an energy / overlap pass over `lanes` chunks of 16 columns
inline unsigned reduce_blocks(long long lanes) {
    const long long b = (lanes + 255) / 256;
    return (unsigned)(b < kEnergyBlocks ? b : kEnergyBlocks);
}

}  // namespace

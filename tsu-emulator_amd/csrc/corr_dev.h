// corr_dev.h -- axis profiles and k_min Fourier modes of a spin plane or of the product of two ("Correlation
// length"): what the second-moment correlation length xi_L needs, for single lattices and for every slot of a tempering ladder.
// Dimension-blind like reduce_dev.h: a plane is `nrows` rows of `pitch` bytes of which the first `cols` count, row rho = z lrows + r
// (2-D: lrows = nrows, one layer, no layer profile).  Everything here has internal linkage.
//
// Profile pass.  f = s (one plane) or s^a s^b (two); P_c[c] = sum over rows, P_r[r] = sum over layers and columns, P_z[z] = sum over
// the layer.  Integer accumulation only, so the result does not depend on the schedule: exact int64 profiles, the same on every run.
// The columns are cut into tiles of 4096 (blockIdx.x), the rows into bands of consecutive steps (blockIdx.y), a step being 256 / L
// consecutive rows of L lanes, L = the power of two >= the tile's chunks of 16 columns: a lane keeps its chunk column for the whole
// band, so the 16 column sums stay in registers until the band ends and then take one LDS add each (bin of column 16 q + i at
// i * 256 + q: consecutive lanes, consecutive banks), and the workgroup flushes the tile's bins with one 64-bit global atomic per
// column.  A row's lanes sit in one wave while L <= 64: a xor-shuffle tree gives the row sum; wider rows add one partial per wave.
// Row sums go to P_r with one global atomic each; the layer sum is kept by the row's first lane while z does not change.  The pass
// reads 1 B per site (2 B for a pair) in 16 B chunks as pair_lane does, and nothing else of that size.
//
// Mode pass.  F_d = sum_x P_d[x] (cos_d[x] + i sin_d[x]) for each periodic axis from host-made tables: thread t of 256 adds the terms
// x = t, t + 256, ... in ascending order from 0.0, then block_sum's fixed tree; no contraction, so the products and sums round as
// NumPy's (tests/helpers/correlation_twin.py restates the order).
#pragma once
#include "reduce_dev.h"

namespace {

constexpr int kProfTileChunks = 256;                 // chunks of 16 columns in a column tile
constexpr int kProfTileCols = 16 * kProfTileChunks;  // 4096 int32 bins: 16 KiB of LDS a workgroup

struct ProfArgs {
    long long pitch_a, pitch_b, nrows;
    int lrows;   // rows of a layer
    int cols;
    int lshift;  // log2 L
    int steps;   // steps of a band
    int has_z;   // the layer profile exists (3-D)
};

// c + the sum of the four products of the signed bytes of a and b (v_dot4_i32_i8), exact in int32
__device__ __forceinline__ int dot4(uint32_t a, uint32_t b, int c) { return __builtin_amdgcn_sdot4((int)a, (int)b, c, false); }

// the profiles of one plane pair in the layout [P_z (nrows / lrows, if has_z) | P_r (lrows) | P_c (cols)], added into zeroed `out`
__device__ __forceinline__ void profile_block(const int8_t* __restrict__ a, const int8_t* __restrict__ b, const ProfArgs& p,
                                              long long* __restrict__ out) {
    __shared__ int bins[kProfTileCols];
    long long* const pz = out;
    long long* const pr = out + (p.has_z ? p.nrows / p.lrows : 0);
    long long* const pc = pr + p.lrows;
    const int tid = threadIdx.x;
    const int L = 1 << p.lshift, rs = 256 >> p.lshift;
    const int ql = tid & (L - 1), rl = tid >> p.lshift;
    const int q = (int)blockIdx.x * kProfTileChunks + ql;
    const int c0 = 16 * q;
    const bool live = c0 < p.cols;
    const int group = L < 64 ? L : 64;  // lanes of a wave that share a row
    const bool lead = (tid & (group - 1)) == 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) bins[i * kProfTileChunks + tid] = 0;
    __syncthreads();
    int acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0;
    // Columns >= cols never count: the lane clears their bytes of plane a once, so that they add 0 to every sum, and one plane is
    // the product with a plane of ones.  (Masking each product with a select instead, `c0 + i < cols ? sa * sb : 0`, and summing
    // those made the compiler fuse selects and products into one v_dot4c that took a row sum one too low.)
    uint32_t keep[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int n = p.cols - (c0 + 4 * w);  // columns of this word that count
        keep[w] = n >= 4 ? 0xFFFFFFFFu : (n <= 0 ? 0u : (1u << (8 * n)) - 1u);
    }
    const uint4 ones = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
    long long zcur = -1, zsum = 0;
    const long long step0 = (long long)blockIdx.y * p.steps;
    for (int k = 0; k < p.steps; ++k) {
        const long long rho = (step0 + k) * rs + rl;
        const bool row = rho < p.nrows;
        int cs = 0;
        if (live && row) {
            uint4 va = *reinterpret_cast<const uint4*>(a + rho * p.pitch_a + c0);
            va.x &= keep[0], va.y &= keep[1], va.z &= keep[2], va.w &= keep[3];
            uint4 vb = ones;
            if (b) vb = *reinterpret_cast<const uint4*>(b + rho * p.pitch_b + c0);
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] += sbyte(va, i) * sbyte(vb, i);
            cs = dot4(va.x, vb.x, dot4(va.y, vb.y, dot4(va.z, vb.z, dot4(va.w, vb.w, 0))));
        }
        for (int off = group >> 1; off > 0; off >>= 1) cs += __shfl_xor(cs, off, 64);
        if (lead && row) {
            if (cs) atomicAdd(reinterpret_cast<unsigned long long*>(pr + rho % p.lrows), (unsigned long long)(long long)cs);
            if (p.has_z) {
                const long long z = rho / p.lrows;
                if (z != zcur) {
                    if (zsum) atomicAdd(reinterpret_cast<unsigned long long*>(pz + zcur), (unsigned long long)zsum);
                    zcur = z;
                    zsum = 0;
                }
                zsum += cs;
            }
        }
    }
    if (zsum) atomicAdd(reinterpret_cast<unsigned long long*>(pz + zcur), (unsigned long long)zsum);
    if (live) {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (acc[i]) atomicAdd(&bins[i * kProfTileChunks + ql], acc[i]);
    }
    __syncthreads();
    const int tile0 = (int)blockIdx.x * kProfTileCols;
    const int ncols = p.cols - tile0 < kProfTileCols ? p.cols - tile0 : kProfTileCols;
    for (int c = tid; c < ncols; c += 256) {
        const int v = bins[(c & 15) * kProfTileChunks + (c >> 4)];
        if (v) atomicAdd(reinterpret_cast<unsigned long long*>(pc + tile0 + c), (unsigned long long)(long long)v);
    }
}

// grid (column tiles, row bands): one plane (b == nullptr) or the product of two
__global__ __launch_bounds__(256) void profile_pass(const int8_t* __restrict__ a, const int8_t* __restrict__ b, ProfArgs p,
                                                    long long* __restrict__ out) {
    profile_block(a, b, p, out);
}

// grid (column tiles, row bands, S R): the walker of ladder 0 of sample z / R at slot z % R, times the walker of ladder 1 there if
// there are two ladders, into out[z * stride ..] (zeroed scratch [sample][slot]); the tables are [sample][ladder][..]
__global__ __launch_bounds__(256) void pt_profile(int8_t* const* __restrict__ s, const int32_t* __restrict__ was, int R, int nl,
                                                  ProfArgs p, long long* __restrict__ out, long long stride) {
    const int z = blockIdx.z, smp = z / R, i = z - smp * R;
    s += (size_t)smp * nl * R;
    was += (size_t)smp * nl * R;
    profile_block(s[was[i]], nl == 2 ? s[R + was[R + i]] : nullptr, p, out + z * stride);
}

struct ModeArgs {
    int n;               // periodic axes
    int off[3], len[3];  // where axis k's profile starts in a slot's row of the scratch, and its length
    const double* cs[3];
    const double* sn[3];
};

// grid (2 n, S R): block (2 k + im, y = (sample, slot)) writes Re / Im F of periodic axis k into out[y][k][im]
__global__ __launch_bounds__(256) void pt_modes(const long long* __restrict__ prof, long long stride, ModeArgs m,
                                                double* __restrict__ out) {
#pragma clang fp contract(off)
    const int k = blockIdx.x >> 1, im = blockIdx.x & 1;
    const long long* P = prof + blockIdx.y * stride + m.off[k];
    const double* tab = im ? m.sn[k] : m.cs[k];
    double e = 0.0;
    for (int x = threadIdx.x; x < m.len[k]; x += 256) e += (double)P[x] * tab[x];
    const double v = block_sum(e);
    if (threadIdx.x == 0) out[((size_t)blockIdx.y * m.n + k) * 2 + im] = v;
}

// the launch shape of a profile pass over `slots` plane pairs
inline dim3 profile_plan(ProfArgs& p, long long pitch_a, long long pitch_b, long long nrows, int lrows, int cols, int has_z,
                         unsigned slots) {
    const int nchunks = (cols + 15) / 16;
    const int tiles = (nchunks + kProfTileChunks - 1) / kProfTileChunks;
    const int per_tile = nchunks < kProfTileChunks ? nchunks : kProfTileChunks;
    int lshift = 0;
    while ((1 << lshift) < per_tile) ++lshift;
    const long long rs = 256 >> lshift;
    const long long nsteps = (nrows + rs - 1) / rs;
    // bands of about 8 steps, at least 256 bands where the rows allow it and at most 1024
    long long bands = (nsteps + 7) / 8;
    if (bands < 256) bands = nsteps < 256 ? nsteps : 256;
    if (bands > 1024) bands = 1024;
    const long long steps = (nsteps + bands - 1) / bands;
    bands = (nsteps + steps - 1) / steps;
    p.pitch_a = pitch_a;
    p.pitch_b = pitch_b;
    p.nrows = nrows;
    p.lrows = lrows;
    p.cols = cols;
    p.lshift = lshift;
    p.steps = (int)steps;
    p.has_z = has_z;
    return dim3((unsigned)tiles, (unsigned)bands, slots);
}

}  // namespace

// ising2d_disorder.hip -- K7: heat-bath sweeps of a 2-D lattice with per-bond couplings and per-site fields (gfx950).
//
// Quenched disorder on the lattice handle: J_right[r][c] (bond (r, c)-(r, c+1), wrapping to column 0 on a periodic lattice),
// J_down[r][c] (bond (r, c)-(r+1, c), wrapping to row 0) and h[r][c], fp32, row-major.  Device copies use the spin buffer's
// pitch (in elements), pad columns 0.  Decision rule (the bit-exact contract):
//   f   = (((J_down[r-1][c] s_up + J_down[r][c] s_down) + J_right[r][c-1] s_left) + J_right[r][c] s_right) + h[r][c] in float64,
//         a missing neighbour of an open lattice skipped (no +0.0);  x = 2 f / T;  p = sigmoid(x) clamped at +-20;
//   thr = floor(p 2^32 + 1/2);  the site becomes +1 iff u < thr, u = K1's own 32-bit site uniform (same counters, same tags:
//         hi16 = half (m & 1) of Philox(c >> 4, r, hs, TAG_ISING_HI | replica << 8)[m >> 1] ^ 0x8000, m = (c >> 1) & 7; lo16
//         from TAG_ISING_LO, drawn only when hi16 ties with thr's top 16 bits).
// With the 25-entry table replaced by this per-site threshold, a constant dyadic (J, h) gives K1's spins bit for bit.
//
// k7_sweep: one launch per half-sweep, one lane per octet (16 consecutive columns of one row = 8 sites of the colour, the
// unit of one Philox block), 64 x 4 lanes per workgroup = one row per wave, so the column parity of the colour is uniform
// in a wave.  The lane screens its 8 sites in fp32 and only takes the float64 threshold of the contract where the fp32
// probability lies within a margin of the hi16 uniform (see screen() for the bound).  The spins are updated in place (a
// colour reads only the other colour), 16-byte masked stores, pad bytes untouched.  Every whole lattice K1 takes runs here
// (one-row and one-column lattices included); slabs are refused.
//
// Bytes: per half-sweep the launch reads every byte of the three disorder rows it touches (12 B per site: the lines hold both
// colours) and the spins (~3 B per site, up / down rows from L2), writes 1 B per site: ~28 B per site and sweep against the
// 2 B + 12 B / s of a tile-resident design.
//
// k7_energy + k7_energy_final: E = -sum_bonds J s s' - sum h s in float64, per-workgroup partials then one workgroup
// summing them in a fixed order (the same bits on every call).  k7_overlap: q = sum s^a s^b (integer, vector atomics).
//
// Parallel tempering (tsu_pt2d_*): ladders of R walkers on ONE disorder ("Parallel tempering (K7)").
// k7_pt_sweep is k7_sweep for a group of W walkers per lane: the octet's disorder is loaded once and every walker of the group
// takes K7's decision at the temperature of its slot (a device table the swap kernel keeps), so the 24 B per site of disorder
// a sweep reads are shared by W walkers.  k7_pt_energy / k7_pt_energy_final run k7_energy's decomposition per walker (the same
// bits as the single-lattice call) and sum the spins alongside; k7_pt_swap makes the reference's sequential swap pass per ladder
// on the device; k7_pt_overlap records q of the two ladders' walkers at each slot.  No host value changes between rounds: a
// run of many rounds is enqueued without a synchronisation.  The handle itself is declared in ising2d_pt.h; the replica cluster
// moves a round may end its sweeps with live in ising2d_icm.hip (the pt2d_icm_* hooks below).
#include <cmath>
#include <cstdlib>
#include <vector>

#include "dense.h"
#include "disorder_dev.h"
#include "ising2d.h"
#include "ising2d_pt.h"

namespace {

constexpr int kEnergyBlocks = 1024;  // fixed partial count: the summation order depends on the shape only

struct K7Params {
    int8_t* s;           // owned row 0 of the current spin buffer
    const float* jr;     // J_right, J_down, h: row pitch = `pitch` elements
    const float* jd;
    const float* h;
    long long pitch;
    int rows, cols, periodic;
    float c32;           // fl32(2 / T): the screen's scale
    double T;
    uint32_t k0, k1, hs, tag_hi, tag_lo;
};

// sbyte, fat, load16f, exact_thr and screen (with the derivation of its margin) live in disorder_dev.h, shared with K8

// one octet of the colour whose sites sit at chunk positions PAR, PAR + 2, ..
template <int PAR>
__device__ __forceinline__ void k7_octet(const K7Params& p, int r, int q) {
    const long long row = (long long)r * p.pitch;
    const int c0 = 16 * q;
    const bool has_up = r > 0 || p.periodic, has_dn = r + 1 < p.rows || p.periodic;
    const long long rowu = (long long)(r > 0 ? r - 1 : p.rows - 1) * p.pitch;
    const long long rowd = (long long)(r + 1 < p.rows ? r + 1 : 0) * p.pitch;
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    const uint4 C = *reinterpret_cast<const uint4*>(p.s + row + c0);
    const uint4 U = has_up ? *reinterpret_cast<const uint4*>(p.s + rowu + c0) : zero4;
    const uint4 D = has_dn ? *reinterpret_cast<const uint4*>(p.s + rowd + c0) : zero4;
    float4 jr[4], jd[4], ju[4], hh[4];
    load16f(p.jr + row + c0, jr);
    load16f(p.jd + row + c0, jd);
    load16f(p.h + row + c0, hh);
    if (has_up) load16f(p.jd + rowu + c0, ju);
    else
        for (int k = 0; k < 4; ++k) ju[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    // column c0 - 1 (left of position 0), column c0 + 16 (right of position 15), column 0 (right of the last column, periodic)
    const bool has_prev = q > 0 || p.periodic;
    const int cprev = q > 0 ? c0 - 1 : p.cols - 1;
    const int s_prev = has_prev ? (int)p.s[row + cprev] : 0;
    const float j_prev = has_prev ? p.jr[row + cprev] : 0.0f;
    const int s_next = (c0 + 16 < p.cols) ? (int)p.s[row + c0 + 16] : 0;
    const int s_first = p.periodic ? (int)p.s[row] : 0;

    const u32x4 w = tsu_philox((uint32_t)q, (uint32_t)r, p.hs, p.tag_hi, p.k0, p.k1);
    const uint32_t wv[4] = {w.x, w.y, w.z, w.w};
    bool have_lo = false;
    uint32_t lv[4] = {0, 0, 0, 0};
    uint32_t out[4] = {C.x, C.y, C.z, C.w};
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int i = 2 * m + PAR, c = c0 + i;
        if (c >= p.cols) break;
        const bool has_left = i > 0 || has_prev, has_right = c + 1 < p.cols || p.periodic;
        const int su = sbyte(U, i), sd = sbyte(D, i);
        const int sl = i > 0 ? sbyte(C, i - 1) : s_prev;
        const int sr = c + 1 < p.cols ? (i < 15 ? sbyte(C, i + 1) : s_next) : s_first;
        const float Ju = has_up ? fat(ju, i) : 0.0f, Jd = has_dn ? fat(jd, i) : 0.0f;
        const float Jl = has_left ? (i > 0 ? fat(jr, i - 1) : j_prev) : 0.0f;
        const float Jr = has_right ? fat(jr, i) : 0.0f;
        const float hf = fat(hh, i);
        // missing neighbours carry J = 0 here: exact in fp32, and the screen only needs a bound
        const float f32 = (((Ju * (float)su + Jd * (float)sd) + Jl * (float)sl) + Jr * (float)sr) + hf;
        const float a32 = fabsf(Ju) + fabsf(Jd) + fabsf(Jl) + fabsf(Jr) + fabsf(hf);
        const uint32_t hi = ((wv[m >> 1] >> (16 * (m & 1))) & 0xFFFFu) ^ 0x8000u;
        int dec = screen(f32, a32, p.c32, hi);
        if (dec == 0) {
            // the contract's sum: neighbours in the order up, down, left, right, a missing one skipped, then h
            double f = 0.0;
            bool any = false;
            if (has_up) { f = (double)Ju * su; any = true; }
            if (has_dn) { f = any ? f + (double)Jd * sd : (double)Jd * sd; any = true; }
            if (has_left) { f = any ? f + (double)Jl * sl : (double)Jl * sl; any = true; }
            if (has_right) { f = any ? f + (double)Jr * sr : (double)Jr * sr; any = true; }
            f = any ? f + (double)hf : (double)hf;
            const uint64_t thr = exact_thr(f, p.T);
            const uint32_t thi = (uint32_t)(thr >> 16);
            bool accept = hi < thi;
            if (hi == thi) {  // tie on the top 16 bits: the low half, as K1 draws it
                if (!have_lo) {
                    const u32x4 l = tsu_philox((uint32_t)q, (uint32_t)r, p.hs, p.tag_lo, p.k0, p.k1);
                    lv[0] = l.x; lv[1] = l.y; lv[2] = l.z; lv[3] = l.w;
                    have_lo = true;
                }
                const uint32_t lo = (lv[m >> 1] >> (16 * (m & 1))) & 0xFFFFu;
                accept = (((uint64_t)hi << 16) | lo) < thr;
            }
            dec = accept ? 1 : -1;
        }
        const uint32_t b = dec > 0 ? 0x01u : 0xFFu;
        const int sh = 8 * (i & 3);
        out[i >> 2] = (out[i >> 2] & ~(0xFFu << sh)) | (b << sh);
    }
    *reinterpret_cast<uint4*>(p.s + row + c0) = make_uint4(out[0], out[1], out[2], out[3]);
}

// grid (ceil(nchunks / 64), ceil(rows / 4)), 64 x 4 lanes: lane = octet q of row r
__global__ __launch_bounds__(256) void k7_sweep(K7Params p, int colour) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    const int r = blockIdx.y * 4 + threadIdx.y;
    if (r >= p.rows || 16 * q >= p.cols) return;
    if (((r + colour) & 1) == 0) k7_octet<0>(p, r, q);
    else k7_octet<1>(p, r, q);
}

// E partial of a lane: lane = chunk (r, q), grid-stride over blockIdx.x in a fixed order; ssum = the lane's sum of spins
__device__ __forceinline__ double k7_energy_lane(const K7Params& p, long long& ssum) {
    const int nchunks = (p.cols + 15) >> 4;
    const long long total = (long long)p.rows * nchunks;
    double e = 0.0;
    long long m = 0;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const int r = (int)(t / nchunks), q = (int)(t - (long long)r * nchunks);
        const long long row = (long long)r * p.pitch;
        const bool has_dn = r + 1 < p.rows || p.periodic;
        const long long rowd = (long long)(r + 1 < p.rows ? r + 1 : 0) * p.pitch;
        for (int i = 0; i < 16; ++i) {
            const int c = 16 * q + i;
            if (c >= p.cols) break;
            const int s = p.s[row + c];
            double l = (double)p.h[row + c];
            if (c + 1 < p.cols || p.periodic) l += (double)p.jr[row + c] * p.s[row + (c + 1 < p.cols ? c + 1 : 0)];
            if (has_dn) l += (double)p.jd[row + c] * p.s[rowd + c];
            e += s * l;
            m += s;
        }
    }
    ssum = m;
    return e;
}

// workgroup sum of 256 lanes: fixed shuffle tree, then the four waves in a fixed order (every thread gets it).  Each of these two
// helpers owns one __shared__ array and ends without a barrier: a kernel may call each of them once (a second call would write
// wpart while slower threads still read the first result).
__device__ __forceinline__ double k7_block_sum(double e) {
    for (int off = 32; off > 0; off >>= 1) e += __shfl_down(e, off, 64);
    __shared__ double wpart[4];
    if ((threadIdx.x & 63) == 0) wpart[threadIdx.x >> 6] = e;
    __syncthreads();
    return (wpart[0] + wpart[1]) + (wpart[2] + wpart[3]);
}

__device__ __forceinline__ long long k7_block_isum(long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __shared__ long long wpart[4];
    if ((threadIdx.x & 63) == 0) wpart[threadIdx.x >> 6] = v;
    __syncthreads();
    return wpart[0] + wpart[1] + wpart[2] + wpart[3];
}

// E partials: one per workgroup
__global__ __launch_bounds__(256) void k7_energy(K7Params p, double* __restrict__ part) {
    long long m;
    const double e = k7_block_sum(k7_energy_lane(p, m));
    if (threadIdx.x == 0) part[blockIdx.x] = e;
}

// -(sum of the n partials), in a fixed order (every thread gets it)
__device__ __forceinline__ double k7_final_sum(const double* __restrict__ part, int n) {
    double e = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) e += part[i];
    return -k7_block_sum(e);
}

// one workgroup: out[0] = E
__global__ __launch_bounds__(256) void k7_energy_final(const double* __restrict__ part, int n, double* __restrict__ out) {
    const double e = k7_final_sum(part, n);
    if (threadIdx.x == 0) out[0] = e;
}

// a lane's share of q = sum over sites of s^a s^b (columns < cols only)
__device__ __forceinline__ long long k7_overlap_lane(const int8_t* __restrict__ a, const int8_t* __restrict__ b, long long pitch_a,
                                                     long long pitch_b, int rows, int cols) {
    const int nchunks = (cols + 15) >> 4;
    const long long total = (long long)rows * nchunks;
    long long sum = 0;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const int r = (int)(t / nchunks), q = (int)(t - (long long)r * nchunks);
        const uint4 va = *reinterpret_cast<const uint4*>(a + r * pitch_a + 16 * q);
        const uint4 vb = *reinterpret_cast<const uint4*>(b + r * pitch_b + 16 * q);
        int cs = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (16 * q + i < cols) cs += sbyte(va, i) * sbyte(vb, i);
        sum += cs;
    }
    return sum;
}

// q, one 64-bit vector atomic per workgroup
__global__ __launch_bounds__(256) void k7_overlap(const int8_t* __restrict__ a, const int8_t* __restrict__ b, long long pitch_a,
                                                  long long pitch_b, int rows, int cols, long long* __restrict__ acc) {
    const long long v = k7_block_isum(k7_overlap_lane(a, b, pitch_a, pitch_b, rows, cols));
    if (threadIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long*>(acc), (unsigned long long)v);
}

// ------------------------------------------------------------------ parallel tempering
// PTSwap, pt_arrive, k7_pt_swap and the round-trip flags live in pt_dev.h, shared with the 3-D ladders (ising3d.hip)

struct PTParams {
    int8_t* const* s;     // walker g = ladder * R + w -> owned row 0 of its spin plane (one pitch for all)
    const uint32_t* key;  // walker -> Philox key (k0, k1) of seed + g
    const int32_t* slot;  // walker -> its slot in its ladder
    const double* T;      // slot -> T
    const float* c32;     // slot -> fl32(2 / T)
    const float* jr;      // the one disorder (K7Params layout)
    const float* jd;
    const float* h;
    long long pitch;
    int rows, cols, periodic;
    int nw, W;            // walkers; walkers per lane (group z of the grid: walkers [z W, z W + W))
    uint32_t hs;
};

// k7_octet for the walkers [g0, g1): the colour's couplings and fields are loaded once, then each walker takes the same
// decision as k7_octet at the temperature of its slot, with its own key (replica 0)
template <int PAR>
__device__ __forceinline__ void k7_pt_octet(const PTParams& p, int r, int q, int g0, int g1) {
    const long long row = (long long)r * p.pitch;
    const int c0 = 16 * q;
    const bool has_up = r > 0 || p.periodic, has_dn = r + 1 < p.rows || p.periodic;
    const long long rowu = (long long)(r > 0 ? r - 1 : p.rows - 1) * p.pitch;
    const long long rowd = (long long)(r + 1 < p.rows ? r + 1 : 0) * p.pitch;
    const bool has_prev = q > 0 || p.periodic;
    const int cprev = q > 0 ? c0 - 1 : p.cols - 1;
    // the colour's 8 sites: J to the up, down, left and right neighbour (0 where it is missing), h, and the screen's sum of |terms|
    float Ju[8], Jd[8], Jl[8], Jr[8], hf[8], a32[8];
    {
        float4 jr[4], jd[4], ju[4], hh[4];
        load16f(p.jr + row + c0, jr);
        load16f(p.jd + row + c0, jd);
        load16f(p.h + row + c0, hh);
        if (has_up) load16f(p.jd + rowu + c0, ju);
        else
            for (int k = 0; k < 4; ++k) ju[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        const float j_prev = has_prev ? p.jr[row + cprev] : 0.0f;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int i = 2 * m + PAR, c = c0 + i;
            const bool has_left = i > 0 || has_prev, has_right = c + 1 < p.cols || p.periodic;
            Ju[m] = has_up ? fat(ju, i) : 0.0f;
            Jd[m] = has_dn ? fat(jd, i) : 0.0f;
            Jl[m] = has_left ? (i > 0 ? fat(jr, i - 1) : j_prev) : 0.0f;
            Jr[m] = has_right ? fat(jr, i) : 0.0f;
            hf[m] = fat(hh, i);
            a32[m] = fabsf(Ju[m]) + fabsf(Jd[m]) + fabsf(Jl[m]) + fabsf(Jr[m]) + fabsf(hf[m]);
        }
    }
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
#pragma unroll 1
    for (int g = g0; g < g1; ++g) {
        int8_t* const s = p.s[g];
        const int slot = p.slot[g];
        const double T = p.T[slot];
        const float c32 = p.c32[slot];
        const uint32_t k0 = p.key[2 * g], k1 = p.key[2 * g + 1];
        const uint4 C = *reinterpret_cast<const uint4*>(s + row + c0);
        const uint4 U = has_up ? *reinterpret_cast<const uint4*>(s + rowu + c0) : zero4;
        const uint4 D = has_dn ? *reinterpret_cast<const uint4*>(s + rowd + c0) : zero4;
        const int s_prev = has_prev ? (int)s[row + cprev] : 0;
        const int s_next = (c0 + 16 < p.cols) ? (int)s[row + c0 + 16] : 0;
        const int s_first = p.periodic ? (int)s[row] : 0;
        const u32x4 w = tsu_philox((uint32_t)q, (uint32_t)r, p.hs, TSU_TAG_ISING_HI, k0, k1);
        const uint32_t wv[4] = {w.x, w.y, w.z, w.w};
        bool have_lo = false;
        uint32_t lv[4] = {0, 0, 0, 0};
        uint32_t out[4] = {C.x, C.y, C.z, C.w};
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int i = 2 * m + PAR, c = c0 + i;
            if (c >= p.cols) break;
            const bool has_left = i > 0 || has_prev, has_right = c + 1 < p.cols || p.periodic;
            const int su = sbyte(U, i), sd = sbyte(D, i);
            const int sl = i > 0 ? sbyte(C, i - 1) : s_prev;
            const int sr = c + 1 < p.cols ? (i < 15 ? sbyte(C, i + 1) : s_next) : s_first;
            const float f32 = (((Ju[m] * (float)su + Jd[m] * (float)sd) + Jl[m] * (float)sl) + Jr[m] * (float)sr) + hf[m];
            const uint32_t hi = ((wv[m >> 1] >> (16 * (m & 1))) & 0xFFFFu) ^ 0x8000u;
            int dec = screen(f32, a32[m], c32, hi);
            if (dec == 0) {
                // the contract's sum: neighbours in the order up, down, left, right, a missing one skipped, then h
                double f = 0.0;
                bool any = false;
                if (has_up) { f = (double)Ju[m] * su; any = true; }
                if (has_dn) { f = any ? f + (double)Jd[m] * sd : (double)Jd[m] * sd; any = true; }
                if (has_left) { f = any ? f + (double)Jl[m] * sl : (double)Jl[m] * sl; any = true; }
                if (has_right) { f = any ? f + (double)Jr[m] * sr : (double)Jr[m] * sr; any = true; }
                f = any ? f + (double)hf[m] : (double)hf[m];
                const uint64_t thr = exact_thr(f, T);
                const uint32_t thi = (uint32_t)(thr >> 16);
                bool accept = hi < thi;
                if (hi == thi) {  // tie on the top 16 bits: the low half, as K1 draws it
                    if (!have_lo) {
                        const u32x4 l = tsu_philox((uint32_t)q, (uint32_t)r, p.hs, TSU_TAG_ISING_LO, k0, k1);
                        lv[0] = l.x; lv[1] = l.y; lv[2] = l.z; lv[3] = l.w;
                        have_lo = true;
                    }
                    const uint32_t lo = (lv[m >> 1] >> (16 * (m & 1))) & 0xFFFFu;
                    accept = (((uint64_t)hi << 16) | lo) < thr;
                }
                dec = accept ? 1 : -1;
            }
            const uint32_t b = dec > 0 ? 0x01u : 0xFFu;
            const int sh = 8 * (i & 3);
            out[i >> 2] = (out[i >> 2] & ~(0xFFu << sh)) | (b << sh);
        }
        *reinterpret_cast<uint4*>(s + row + c0) = make_uint4(out[0], out[1], out[2], out[3]);
    }
}

// grid (ceil(nchunks / 64), ceil(rows / 4), ceil(nw / W)), 64 x 4 lanes: lane = octet q of row r for the walkers of group z
__global__ __launch_bounds__(256) void k7_pt_sweep(PTParams p, int colour) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    const int r = blockIdx.y * 4 + threadIdx.y;
    if (r >= p.rows || 16 * q >= p.cols) return;
    const int g0 = blockIdx.z * p.W, g1 = min(g0 + p.W, p.nw);
    if (((r + colour) & 1) == 0) k7_pt_octet<0>(p, r, q, g0, g1);
    else k7_pt_octet<1>(p, r, q, g0, g1);
}

__device__ __forceinline__ K7Params pt_walker_params(const PTParams& pp, int g) {
    K7Params p;
    p.s = pp.s[g];
    p.jr = pp.jr;
    p.jd = pp.jd;
    p.h = pp.h;
    p.pitch = pp.pitch;
    p.rows = pp.rows;
    p.cols = pp.cols;
    p.periodic = pp.periodic;
    p.c32 = 0.0f;
    p.T = 0.0;
    p.k0 = p.k1 = p.hs = p.tag_hi = p.tag_lo = 0;
    return p;
}

// grid (blocks_for(lattice), nw): workgroup x of walker y computes k7_energy's partial x of that walker alone, and its sum of spins
__global__ __launch_bounds__(256) void k7_pt_energy(PTParams pp, double* __restrict__ part, long long* __restrict__ ipart) {
    long long m;
    const double e = k7_block_sum(k7_energy_lane(pt_walker_params(pp, blockIdx.y), m));
    const long long ms = k7_block_isum(m);
    if (threadIdx.x == 0) {
        part[(size_t)blockIdx.y * kEnergyBlocks + blockIdx.x] = e;
        ipart[(size_t)blockIdx.y * kEnergyBlocks + blockIdx.x] = ms;
    }
}

// one workgroup per walker: E as k7_energy_final sums it, and the sum of spins
__global__ __launch_bounds__(256) void k7_pt_energy_final(const double* __restrict__ part, const long long* __restrict__ ipart, int n,
                                                          double* __restrict__ E, long long* __restrict__ M) {
    const size_t base = (size_t)blockIdx.x * kEnergyBlocks;
    const double e = k7_final_sum(part + base, n);
    long long m = 0;
    for (int i = threadIdx.x; i < n; i += 256) m += ipart[base + i];
    const long long ms = k7_block_isum(m);
    if (threadIdx.x == 0) {
        E[blockIdx.x] = e;
        M[blockIdx.x] = ms;
    }
}

// grid (blocks_for(lattice), R): q of the two ladders' walkers at slot y, added into out[y]
__global__ __launch_bounds__(256) void k7_pt_overlap(int8_t* const* __restrict__ s, const int32_t* __restrict__ was, int R,
                                                     long long pitch, int rows, int cols, long long* __restrict__ out) {
    const int i = blockIdx.y;
    const long long v = k7_block_isum(k7_overlap_lane(s[was[i]], s[R + was[R + i]], pitch, pitch, rows, cols));
    if (threadIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long*>(out + i), (unsigned long long)v);
}

bool whole_lattice(const tsu_ising2d* L) { return L->ghost == 0 && L->row0 == 0 && L->total_rows == L->rows; }

K7Params make_params(const tsu_ising2d* L) {
    K7Params p;
    const size_t plane = (size_t)L->rows * L->pitch;
    p.s = L->alloc[L->cur];
    p.jr = L->d_dis;
    p.jd = L->d_dis ? L->d_dis + plane : nullptr;
    p.h = L->d_dis ? L->d_dis + 2 * plane : nullptr;
    p.pitch = (long long)L->pitch;
    p.rows = L->rows;
    p.cols = L->cols;
    p.periodic = L->periodic;
    p.c32 = 0.0f;
    p.T = 0.0;
    p.k0 = p.k1 = p.hs = p.tag_hi = p.tag_lo = 0;
    return p;
}

unsigned blocks_for(const tsu_ising2d* L) {
    const long long work = (long long)L->rows * ((L->cols + 15) / 16);
    const long long b = (work + 255) / 256;
    return (unsigned)(b < kEnergyBlocks ? b : kEnergyBlocks);
}

}  // namespace

namespace {

void pt_free_history(tsu_pt2d* P) {
    void* bufs[] = {P->d_hE, P->d_hM, P->d_hW, P->d_hq};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    P->d_hE = nullptr;
    P->d_hM = nullptr;
    P->d_hW = nullptr;
    P->d_hq = nullptr;
    P->hist_cap = 0;
}

void pt_free(tsu_pt2d* P) {
    void* bufs[] = {P->d_s, P->d_key, P->d_slot, P->d_was, P->d_flag, P->d_T, P->d_c32, P->d_att, P->d_acc,
                    P->d_trips, P->d_part, P->d_ipart, P->d_E, P->d_M};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    pt_free_history(P);
    pt2d_icm_free(P);
    if (P->lat) {
        for (int g = 0; g < P->nw; ++g)
            if (P->lat[g]) (void)tsu_ising2d_destroy(P->lat[g]);
        delete[] P->lat;
    }
    delete P;
}

// every walker at its own slot, the walker at slot 0 "bottom", no attempts, accepts or round trips (synchronises)
int pt_reset(tsu_pt2d* P) {
    tsu_ctx* ctx = P->ctx;
    const int R = P->R, nl = P->nl;
    std::vector<int32_t> ident((size_t)nl * R), flag((size_t)nl * R, kPtNone);
    for (int k = 0; k < nl; ++k) {
        for (int w = 0; w < R; ++w) ident[(size_t)k * R + w] = w;
        flag[(size_t)k * R] = kPtBottom;
    }
    const size_t b = (size_t)nl * R * sizeof(int32_t);
    TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_slot, ident.data(), b, hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_was, ident.data(), b, hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_flag, flag.data(), b, hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_att, 0, (size_t)nl * (R - 1) * sizeof(long long), ctx->stream));
    TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_acc, 0, (size_t)nl * (R - 1) * sizeof(long long), ctx->stream));
    TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_trips, 0, (size_t)nl * R * sizeof(long long), ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    P->sweeps = P->rounds = 0;
    P->hist_rounds = 0;
    return TSU_OK;
}

// Walkers per lane of k7_pt_sweep: the fewest groups that still give >= 1024 lanes per CU (a lane per octet and group), so a
// large lattice reads each octet's disorder once for many walkers and a small one spreads its walkers over the chip.
// TSU_PT_GROUP=w (read per call) forces w.
int pt_group(const tsu_pt2d* P) {
    if (const char* e = getenv("TSU_PT_GROUP")) {
        const int w = atoi(e);
        if (w >= 1) return w < P->nw ? w : P->nw;
    }
    const tsu_ising2d* L = P->lat[0];
    const long long lanes = (long long)L->rows * ((L->cols + 15) / 16);
    const long long want = (long long)(P->ctx->cus > 0 ? P->ctx->cus : 256) * 1024;
    const long long groups = (want + lanes - 1) / lanes;
    if (groups >= P->nw) return 1;
    return (int)((P->nw + groups - 1) / groups);
}

PTParams pt_params(const tsu_pt2d* P) {
    const tsu_ising2d* L = P->lat[0];
    const size_t plane = (size_t)L->rows * L->pitch;
    PTParams p;
    p.s = P->d_s;
    p.key = P->d_key;
    p.slot = P->d_slot;
    p.T = P->d_T;
    p.c32 = P->d_c32;
    p.jr = L->d_dis;
    p.jd = L->d_dis ? L->d_dis + plane : nullptr;
    p.h = L->d_dis ? L->d_dis + 2 * plane : nullptr;
    p.pitch = (long long)L->pitch;
    p.rows = L->rows;
    p.cols = L->cols;
    p.periodic = L->periodic;
    p.nw = P->nw;
    p.W = 1;
    p.hs = 0;
    return p;
}

// every walker's E and sum of spins into d_E / d_M (asynchronous)
void pt_enqueue_energies(tsu_pt2d* P, const PTParams& p) {
    const unsigned blocks = blocks_for(P->lat[0]);
    k7_pt_energy<<<dim3(blocks, (unsigned)P->nw, 1), 256, 0, P->ctx->stream>>>(p, P->d_part, P->d_ipart);
    k7_pt_energy_final<<<(unsigned)P->nw, 256, 0, P->ctx->stream>>>(P->d_part, P->d_ipart, (int)blocks, P->d_E, P->d_M);
}

// the lattice of the walker now at (ladder, slot) (synchronises)
int pt_at(tsu_pt2d* P, int ladder, int slot, const char* what, tsu_ising2d** out) {
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, ladder >= 0 && ladder < P->nl && slot >= 0 && slot < P->R,
                "%s: ladder %d, slot %d out of range (%d ladder(s) of %d temperatures)", what, ladder, slot, P->nl, P->R);
    int32_t w = -1;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(&w, P->d_was + (size_t)ladder * P->R + slot, sizeof(w), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (w < 0 || w >= P->R) return tsu_fail(ctx, TSU_E_HIP, "%s: corrupt slot table (walker %d)", what, (int)w);
    *out = P->lat[ladder * P->R + w];
    return TSU_OK;
}

}  // namespace

extern "C" {

int tsu_ising2d_set_disorder(tsu_ising2d* L, const float* J_right, const float* J_down, const float* h) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, J_right && J_down, "ising2d_set_disorder: J_right and J_down are required (h may be NULL)");
    if (!whole_lattice(L)) return tsu_fail(ctx, TSU_E_UNSUPPORTED, "ising2d_set_disorder: whole lattices only (not a slab)");
    const int rows = L->rows, cols = L->cols;
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            const size_t i = (size_t)r * cols + c;
            TSU_REQUIRE(ctx, std::isfinite(J_right[i]) && std::isfinite(J_down[i]) && (!h || std::isfinite(h[i])),
                        "ising2d_set_disorder: non-finite value at site (%d, %d)", r, c);
            TSU_REQUIRE(ctx, L->periodic || c + 1 < cols || J_right[i] == 0.0f,
                        "ising2d_set_disorder: open lattice: J_right[%d, %d] (last column) must be 0, got %g", r, c, (double)J_right[i]);
            TSU_REQUIRE(ctx, L->periodic || r + 1 < rows || J_down[i] == 0.0f,
                        "ising2d_set_disorder: open lattice: J_down[%d, %d] (last row) must be 0, got %g", r, c, (double)J_down[i]);
        }
    const size_t plane = (size_t)rows * L->pitch;
    if (!L->d_dis) {
        TSU_HIP_TRY(ctx, hipMalloc((void**)&L->d_dis, 3 * plane * sizeof(float)));
        TSU_HIP_TRY(ctx, hipMemsetAsync(L->d_dis, 0, 3 * plane * sizeof(float), ctx->stream));  // pad columns stay 0
    }
    const size_t dpitch = L->pitch * sizeof(float), w = (size_t)cols * sizeof(float);
    TSU_HIP_TRY(ctx, hipMemcpy2DAsync(L->d_dis, dpitch, J_right, w, w, (size_t)rows, hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipMemcpy2DAsync(L->d_dis + plane, dpitch, J_down, w, w, (size_t)rows, hipMemcpyHostToDevice, ctx->stream));
    if (h) TSU_HIP_TRY(ctx, hipMemcpy2DAsync(L->d_dis + 2 * plane, dpitch, h, w, w, (size_t)rows, hipMemcpyHostToDevice, ctx->stream));
    else TSU_HIP_TRY(ctx, hipMemsetAsync(L->d_dis + 2 * plane, 0, plane * sizeof(float), ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    L->have_disorder = 1;
    return TSU_OK;
}

int tsu_ising2d_clear_disorder(tsu_ising2d* L) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    L->have_disorder = 0;  // the buffers stay for the next set_disorder (freed with the handle)
    return TSU_OK;
}

int tsu_ising2d_disorder_sweep(tsu_ising2d* L, double T, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, L->have_disorder, "ising2d_disorder_sweep: call tsu_ising2d_set_disorder first");
    TSU_REQUIRE(ctx, T > 0.0 && std::isfinite(T), "Temperature must be positive");
    TSU_REQUIRE(ctx, n_sweeps >= 0, "ising2d_sweep: n_sweeps must be >= 0");
    TSU_REQUIRE(ctx, (uint64_t)sweep0 + (uint64_t)n_sweeps <= (1ull << 31), "ising2d_sweep: sweep counter overflow");
    if (n_sweeps == 0) return TSU_OK;
    if (L->timing) TSU_HIP_TRY(ctx, hipEventRecord(L->ev0, ctx->stream));
    K7Params p = make_params(L);
    ising2d_set_keys(p, seed, replica);
    p.T = T;
    p.c32 = (float)(2.0 / T);
    const int nchunks = (L->cols + 15) >> 4;
    const dim3 grid((unsigned)((nchunks + 63) / 64), (unsigned)((L->rows + 3) / 4), 1);
    for (int s = 0; s < n_sweeps; ++s)
        for (int colour = 0; colour < 2; ++colour) {
            p.hs = 2u * (sweep0 + (uint32_t)s) + (uint32_t)colour;
            k7_sweep<<<grid, dim3(64, 4, 1), 0, ctx->stream>>>(p, colour);
            L->dis_launches += 1;
        }
    TSU_HIP_TRY(ctx, hipGetLastError());
    if (L->timing) {
        TSU_HIP_TRY(ctx, hipEventRecord(L->ev1, ctx->stream));
        L->timed = 1;
    }
    return TSU_OK;
}

int tsu_ising2d_disorder_energy(tsu_ising2d* L, double* E) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, E, "ising2d_disorder_energy: NULL output");
    TSU_REQUIRE(ctx, L->have_disorder, "ising2d_disorder_energy: call tsu_ising2d_set_disorder first");
    const unsigned blocks = blocks_for(L);
    TSU_HIP_TRY(ctx, ising2d_grow(L->d_dis_part, L->dis_part_cap, (kEnergyBlocks + 1) * sizeof(double)));
    const K7Params p = make_params(L);
    k7_energy<<<blocks, 256, 0, ctx->stream>>>(p, L->d_dis_part);
    k7_energy_final<<<1, 256, 0, ctx->stream>>>(L->d_dis_part, (int)blocks, L->d_dis_part + kEnergyBlocks);
    TSU_HIP_TRY(ctx, hipGetLastError());
    double e = 0.0;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(&e, L->d_dis_part + kEnergyBlocks, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *E = e;
    return ising2d_check_err(L);
}

int tsu_ising2d_overlap(tsu_ising2d* A, tsu_ising2d* B, int64_t* q) {
    TSU_ENTER(A ? A->ctx : nullptr);
    if (!A || !B) return TSU_E_INVALID;
    tsu_ctx* ctx = A->ctx;
    TSU_REQUIRE(ctx, q, "ising2d_overlap: NULL output");
    TSU_REQUIRE(ctx, B->ctx == ctx, "ising2d_overlap: the two lattices belong to different contexts");
    TSU_REQUIRE(ctx, A->rows == B->rows && A->cols == B->cols && A->total_rows == B->total_rows,
                "ising2d_overlap: shapes differ (%d x %d against %d x %d)", A->rows, A->cols, B->rows, B->cols);
    TSU_REQUIRE(ctx, whole_lattice(A) && whole_lattice(B), "ising2d_overlap: whole lattices only (not slabs)");
    TSU_HIP_TRY(ctx, hipMemsetAsync(A->d_obs, 0, sizeof(int64_t), ctx->stream));
    k7_overlap<<<blocks_for(A), 256, 0, ctx->stream>>>(A->alloc[A->cur], B->alloc[B->cur], (long long)A->pitch, (long long)B->pitch,
                                                       A->rows, A->cols, (long long*)A->d_obs);
    TSU_HIP_TRY(ctx, hipGetLastError());
    int64_t h = 0;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(&h, A->d_obs, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *q = h;
    int rc = ising2d_check_err(A);
    return rc != TSU_OK ? rc : ising2d_check_err(B);
}

int tsu_ising2d_disorder_launch_count(tsu_ising2d* L, uint64_t* n) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L || !n) return TSU_E_INVALID;
    *n = L->dis_launches;
    return TSU_OK;
}

// ------------------------------------------------------------------ parallel tempering
int tsu_pt2d_create(tsu_ctx* ctx, int rows, int cols, int periodic, int n_temps, int n_ladders, tsu_pt2d** out) {
    TSU_ENTER(ctx);
    if (!ctx || !out) return TSU_E_INVALID;
    *out = nullptr;
    TSU_REQUIRE(ctx, n_temps >= 2 && n_temps <= kPtMaxTemps, "pt2d_create: n_temps must be in [2, %d], got %d", kPtMaxTemps, n_temps);
    TSU_REQUIRE(ctx, n_ladders == 1 || n_ladders == 2, "pt2d_create: n_ladders must be 1 or 2, got %d", n_ladders);
    tsu_pt2d* P = new (std::nothrow) tsu_pt2d();
    if (!P) return tsu_fail(ctx, TSU_E_NOMEM, "pt2d_create: host allocation failed");
    P->ctx = ctx;
    P->R = n_temps;
    P->nl = n_ladders;
    P->nw = n_temps * n_ladders;
    P->lat = new (std::nothrow) tsu_ising2d*[P->nw]();
    if (!P->lat) {
        pt_free(P);
        return tsu_fail(ctx, TSU_E_NOMEM, "pt2d_create: host allocation failed");
    }
    for (int g = 0; g < P->nw; ++g) {  // every whole lattice K7 takes (the shape checks of tsu_ising2d_create)
        const int rc = tsu_ising2d_create(ctx, rows, cols, periodic, &P->lat[g]);
        if (rc != TSU_OK) {
            pt_free(P);
            return rc;
        }
    }
    const size_t nw = (size_t)P->nw, nlR = (size_t)P->nl * P->R, R = (size_t)P->R;
    hipError_t e = hipSuccess;
    auto alloc = [&e](auto*& ptr, size_t bytes) {
        if (e == hipSuccess) e = hipMalloc((void**)&ptr, bytes);
    };
    alloc(P->d_s, nw * sizeof(int8_t*));
    alloc(P->d_key, 2 * nw * sizeof(uint32_t));
    alloc(P->d_slot, nlR * sizeof(int32_t));
    alloc(P->d_was, nlR * sizeof(int32_t));
    alloc(P->d_flag, nlR * sizeof(int32_t));
    alloc(P->d_T, R * sizeof(double));
    alloc(P->d_c32, R * sizeof(float));
    alloc(P->d_att, (size_t)P->nl * (R - 1) * sizeof(long long));
    alloc(P->d_acc, (size_t)P->nl * (R - 1) * sizeof(long long));
    alloc(P->d_trips, nlR * sizeof(long long));
    alloc(P->d_part, nw * kEnergyBlocks * sizeof(double));
    alloc(P->d_ipart, nw * kEnergyBlocks * sizeof(long long));
    alloc(P->d_E, nw * sizeof(double));
    alloc(P->d_M, nw * sizeof(long long));
    std::vector<int8_t*> planes(nw);
    for (size_t g = 0; g < nw; ++g) planes[g] = P->lat[g]->alloc[P->lat[g]->cur];
    if (e == hipSuccess) e = hipMemcpyAsync(P->d_s, planes.data(), nw * sizeof(int8_t*), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(P->d_key, 0, 2 * nw * sizeof(uint32_t), ctx->stream);
    if (e != hipSuccess) {
        const int rc = tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "pt2d_create: %s", hipGetErrorString(e));
        (void)hipStreamSynchronize(ctx->stream);
        pt_free(P);
        return rc;
    }
    const int rc = pt_reset(P);  // synchronises before `planes` goes
    if (rc != TSU_OK) {
        pt_free(P);
        return rc;
    }
    *out = P;
    return TSU_OK;
}

int tsu_pt2d_destroy(tsu_pt2d* P) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_OK;
    (void)hipStreamSynchronize(P->ctx->stream);
    pt_free(P);
    return TSU_OK;
}

int tsu_pt2d_set_disorder(tsu_pt2d* P, const float* J_right, const float* J_down, const float* h) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    return tsu_ising2d_set_disorder(P->lat[0], J_right, J_down, h);  // stored once, with walker 0's lattice
}

int tsu_pt2d_set_temperatures(tsu_pt2d* P, const double* T) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, T, "pt2d_set_temperatures: NULL temperatures");
    double t[kPtMaxTemps];
    float c[kPtMaxTemps];
    for (int i = 0; i < P->R; ++i) {
        TSU_REQUIRE(ctx, T[i] > 0.0 && std::isfinite(T[i]), "Temperature must be positive (pt2d_set_temperatures: T[%d] = %g)", i, T[i]);
        t[i] = T[i];
        c[i] = (float)(2.0 / T[i]);
    }
    for (int i = 0; i < P->R; ++i) P->h_T[i] = t[i];
    TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_T, t, P->R * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_c32, c, P->R * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    P->have_T = 1;
    return pt2d_icm_slots(P);  // which slots take part in the cluster moves (nothing to do while they are off)
}

int tsu_pt2d_init(tsu_pt2d* P, uint64_t seed, int initial) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, initial == 0 || initial == 1 || initial == -1, "pt2d_init: initial must be 0 (random), 1 (up) or -1 (down), got %d",
                initial);
    std::vector<uint32_t> key(2 * (size_t)P->nw);
    for (int g = 0; g < P->nw; ++g) {
        const uint64_t s = seed + (uint64_t)g;  // temperature_scan's model g
        key[2 * g] = (uint32_t)s;
        key[2 * g + 1] = (uint32_t)(s >> 32);
        const int rc = initial == 0 ? tsu_ising2d_randomize(P->lat[g], s, 0) : tsu_ising2d_fill(P->lat[g], (int8_t)initial);
        if (rc != TSU_OK) return rc;
    }
    TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_key, key.data(), key.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    int rc = pt_reset(P);  // synchronises before `key` goes
    if (rc != TSU_OK) return rc;
    rc = pt2d_icm_reset(P);
    if (rc != TSU_OK) return rc;
    P->key0 = (uint32_t)seed;
    P->key1 = (uint32_t)(seed >> 32);
    P->have_init = 1;
    return TSU_OK;
}

int tsu_pt2d_run(tsu_pt2d* P, int n_rounds, int swap_interval, int do_swap, int record) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    tsu_ising2d* L = P->lat[0];
    TSU_REQUIRE(ctx, L->have_disorder, "pt2d_run: call tsu_pt2d_set_disorder first");
    TSU_REQUIRE(ctx, P->have_T, "pt2d_run: call tsu_pt2d_set_temperatures first");
    TSU_REQUIRE(ctx, P->have_init, "pt2d_run: call tsu_pt2d_init first");
    TSU_REQUIRE(ctx, n_rounds >= 0 && swap_interval >= 1, "pt2d_run: need n_rounds >= 0 and swap_interval >= 1 (got %d, %d)", n_rounds,
                swap_interval);
    TSU_REQUIRE(ctx, (uint64_t)P->sweeps + (uint64_t)n_rounds * (uint64_t)swap_interval <= (1ull << 31), "pt2d_run: sweep counter overflow");
    TSU_REQUIRE(ctx, (uint64_t)P->rounds + (uint64_t)n_rounds <= 0xFFFFFFFFull, "pt2d_run: round counter overflow");
    TSU_REQUIRE(ctx, (uint64_t)P->icm_passes + (uint64_t)n_rounds <= 0xFFFFFFFFull, "pt2d_run: cluster-pass counter overflow");
    const int R = P->R, nl = P->nl;
    if (record && P->hist_cap < (size_t)n_rounds) {
        pt_free_history(P);
        const size_t n = (size_t)n_rounds * nl * R;
        TSU_HIP_TRY(ctx, hipMalloc((void**)&P->d_hE, n * sizeof(double)));
        TSU_HIP_TRY(ctx, hipMalloc((void**)&P->d_hM, n * sizeof(long long)));
        TSU_HIP_TRY(ctx, hipMalloc((void**)&P->d_hW, n * sizeof(int32_t)));
        TSU_HIP_TRY(ctx, hipMalloc((void**)&P->d_hq, (size_t)n_rounds * R * sizeof(long long)));
        P->hist_cap = (size_t)n_rounds;
    }
    // k7_pt_overlap adds into its row: every q row of this run starts at 0
    if (record && nl == 2 && n_rounds > 0)
        TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_hq, 0, (size_t)n_rounds * R * sizeof(long long), ctx->stream));
    P->hist_rounds = record ? n_rounds : 0;
    PTParams p = pt_params(P);
    p.W = pt_group(P);
    const int nchunks = (L->cols + 15) >> 4;
    const dim3 grid((unsigned)((nchunks + 63) / 64), (unsigned)((L->rows + 3) / 4), (unsigned)((P->nw + p.W - 1) / p.W));
    PTSwap sw;
    sw.E = P->d_E;
    sw.M = P->d_M;
    sw.T = P->d_T;
    sw.was = P->d_was;
    sw.slot = P->d_slot;
    sw.flag = P->d_flag;
    sw.att = P->d_att;
    sw.acc = P->d_acc;
    sw.trips = P->d_trips;
    sw.R = R;
    sw.do_swap = do_swap ? 1 : 0;
    sw.k0 = P->key0;
    sw.k1 = P->key1;
    for (int t = 0; t < n_rounds; ++t) {
        for (int s = 0; s < swap_interval; ++s)
            for (int colour = 0; colour < 2; ++colour) {
                p.hs = 2u * (P->sweeps + (uint32_t)s) + (uint32_t)colour;
                k7_pt_sweep<<<grid, dim3(64, 4, 1), 0, ctx->stream>>>(p, colour);
                P->launches += 1;
            }
        P->sweeps += (uint32_t)swap_interval;
        if (P->icm_every >= 1 && P->rounds % (uint32_t)P->icm_every == 0) {  // replica cluster moves: the energies see the moved spins
            const int rc = pt2d_icm_enqueue(P);
            if (rc != TSU_OK) return rc;
        }
        if (do_swap || record) {
            pt_enqueue_energies(P, p);
            const size_t row = (size_t)t * nl * R;
            sw.hE = record ? P->d_hE + row : nullptr;
            sw.hM = record ? P->d_hM + row : nullptr;
            sw.hW = record ? P->d_hW + row : nullptr;
            sw.t = P->rounds;
            k7_pt_swap<<<(unsigned)nl, 64, 0, ctx->stream>>>(sw);
            if (record && nl == 2)
                k7_pt_overlap<<<dim3(blocks_for(L), (unsigned)R, 1), 256, 0, ctx->stream>>>(P->d_s, P->d_was, R, (long long)L->pitch, L->rows,
                                                                                           L->cols, P->d_hq + (size_t)t * R);
        }
        P->rounds += 1;
    }
    TSU_HIP_TRY(ctx, hipGetLastError());
    return TSU_OK;
}

int tsu_pt2d_history(tsu_pt2d* P, double* E, int64_t* M, int64_t* q, int32_t* walker) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    const size_t n = (size_t)P->hist_rounds * P->nl * P->R;
    if (n) {
        if (E) TSU_HIP_TRY(ctx, hipMemcpyAsync(E, P->d_hE, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (M) TSU_HIP_TRY(ctx, hipMemcpyAsync(M, P->d_hM, n * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        if (walker) TSU_HIP_TRY(ctx, hipMemcpyAsync(walker, P->d_hW, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        if (q && P->nl == 2)
            TSU_HIP_TRY(ctx, hipMemcpyAsync(q, P->d_hq, (size_t)P->hist_rounds * P->R * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int tsu_pt2d_stats(tsu_pt2d* P, int64_t* attempts, int64_t* accepts, int64_t* round_trips, int32_t* walker_at_slot, uint64_t* sweep_count,
                   uint64_t* round_count) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    const size_t pairs = (size_t)P->nl * (P->R - 1), nlR = (size_t)P->nl * P->R;
    if (attempts) TSU_HIP_TRY(ctx, hipMemcpyAsync(attempts, P->d_att, pairs * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (accepts) TSU_HIP_TRY(ctx, hipMemcpyAsync(accepts, P->d_acc, pairs * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (round_trips) TSU_HIP_TRY(ctx, hipMemcpyAsync(round_trips, P->d_trips, nlR * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (walker_at_slot)
        TSU_HIP_TRY(ctx, hipMemcpyAsync(walker_at_slot, P->d_was, nlR * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (sweep_count) *sweep_count = P->sweeps;
    if (round_count) *round_count = P->rounds;
    return TSU_OK;
}

int tsu_pt2d_energies(tsu_pt2d* P, double* E, int64_t* sum_s) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, P->lat[0]->have_disorder, "pt2d_energies: call tsu_pt2d_set_disorder first");
    pt_enqueue_energies(P, pt_params(P));
    TSU_HIP_TRY(ctx, hipGetLastError());
    if (E) TSU_HIP_TRY(ctx, hipMemcpyAsync(E, P->d_E, (size_t)P->nw * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (sum_s) TSU_HIP_TRY(ctx, hipMemcpyAsync(sum_s, P->d_M, (size_t)P->nw * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int tsu_pt2d_get_spins(tsu_pt2d* P, int ladder, int slot, int8_t* host) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    TSU_REQUIRE(P->ctx, host, "pt2d_get_spins: NULL output");
    tsu_ising2d* L = nullptr;
    const int rc = pt_at(P, ladder, slot, "pt2d_get_spins", &L);
    return rc != TSU_OK ? rc : tsu_ising2d_get_spins(L, host, 0, L->rows);
}

int tsu_pt2d_set_spins(tsu_pt2d* P, int ladder, int slot, const int8_t* host) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    TSU_REQUIRE(P->ctx, host, "pt2d_set_spins: NULL input");
    tsu_ising2d* L = nullptr;
    const int rc = pt_at(P, ladder, slot, "pt2d_set_spins", &L);
    return rc != TSU_OK ? rc : tsu_ising2d_set_spins(L, host, 0, L->rows);
}

int tsu_pt2d_launch_count(tsu_pt2d* P, uint64_t* n) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P || !n) return TSU_E_INVALID;
    *n = P->launches;
    return TSU_OK;
}

}  // extern "C"

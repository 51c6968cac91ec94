// ising3d.hip -- K8: heat-bath sweeps of a 3-D (cubic) lattice with per-bond couplings and per-site fields (gfx950).
//
// Site (z, r, c) of a D x R x C lattice of +-1 int8 spins, row-major with c fastest.  fp32 arrays of shape (D, R, C):
// J_right[z,r,c] couples (z,r,c)-(z,r,c+1), J_down[z,r,c] couples (z,r,c)-(z,r+1,c), J_layer[z,r,c] couples (z,r,c)-(z+1,r,c),
// h[z,r,c] is the site's field.  One periodic flag per axis (p_z, p_r, p_c); a periodic axis wraps to index 0 and has an even
// length >= 4, on an open axis the last slice of that axis's J is 0.  Device copies: rows of `pitch` elements (cols rounded up
// to 16: every row starts 16-byte aligned), pad columns 0, row rho = z R + r at rho * pitch.
// Decision rule (the bit-exact contract; physical mode):
//   colour of a site = (z + r + c) & 1; sweep t = half-sweep hs = 2 t (colour 0), then hs = 2 t + 1 (colour 1);
//   f   = ((((((J_layer[z-1] s[z-1]) + J_layer[z] s[z+1]) + J_down[r-1] s[r-1]) + J_down[r] s[r+1]) + J_right[c-1] s[c-1])
//         + J_right[c] s[c+1]) + h in float64, a neighbour missing on an open axis skipped (no +0.0);
//   x = 2 f / T;  p = sigmoid(x) clamped at +-20;  thr = floor(p 2^32 + 1/2);  the site becomes +1 iff u < thr;
//   u   = K1's 32-bit site uniform with the global row rho = z R + r in place of r: hi16 = half (m & 1) of
//         Philox(c >> 4, rho, hs, TAG_ISING_HI | replica << 8)[m >> 1] ^ 0x8000, m = (c >> 1) & 7, key = seed; lo16 from
//         TAG_ISING_LO, drawn only when hi16 ties with thr's top 16 bits.  No new tag.
// With D = 1 and p_z = 0 the z terms vanish, rho = r, and the rule is K7's: the spins equal tsu_ising2d_disorder_sweep's.
// randomize gives the spins tsu_ising2d_randomize gives a (D R) x C lattice.
//
// k8_sweep: one launch per half-sweep, in place (a colour reads only the other colour), one lane per octet (16 consecutive
// columns of one row rho = 8 sites of the colour = one Philox block).  A row takes L = min(64, the power of two >= ceil(C / 16))
// lanes, a workgroup of 256 lanes 256 / L consecutive rows; its even local rows go to waves 0 and 1, the odd ones to waves 2
// and 3, so the column parity (z + r + colour) & 1 is uniform in a wave except where a wave straddles two layers (the two
// parities are then taken one after the other; the result does not depend on it).  With C >= 1024 this is K7's shape: one row
// per wave.  The lane loads 16 bytes of its own row, of rows r -+ 1 of the layer and of the same row of layers z -+ 1, 16 floats
// of J_right, J_down, J_layer and h at the site and of J_down[r-1] and J_layer[z-1]; it screens its 8 sites in fp32 and takes
// the float64 threshold (and the lo16 block) only where the screen cannot decide (disorder_dev.h: the bound for seven terms);
// one 16-byte store, the other colour's and the pad bytes written back as read.
//
// Bytes: a half-sweep reads every byte of the four arrays (16 B per site: a line holds both colours; J_down[r-1] and
// J_layer[z-1] are the own rows of other lanes of the launch and come from L2) and the spins (1 B per site from HBM, the four
// neighbour rows from L2), and writes 1 B per site: ~36 B per site and sweep.
//
// k8_energy + energy_final: E = -sum_bonds J s s' - sum h s in float64, a fixed number of per-workgroup partials then one
// workgroup summing them in a fixed order (the same bits on every call).  k8_sum / k8_overlap: sum s and q = sum s^a s^b
// (integers, one 64-bit vector atomic per workgroup).  The workgroup sums, the final sums and the pair lane are reduce_dev.h's,
// shared with K7.  No cooperative launch, no waiting, no atomics on the sweep path.
//
// Parallel tempering (tsu_pt3d_*): ladders of R walkers on ONE disorder ("Parallel tempering in 3-D (K8)").
// k8_pt_sweep is k8_sweep for a group of W walkers per lane (the walker group is the grid's z dimension): the octet's six
// couplings, field and screen bound are staged once and every walker of the group takes k8_octet's decision at the temperature
// of its slot, so the 32 B per site of disorder a sweep reads are shared by W walkers.  k8_pt_energy runs k8_energy's
// decomposition per walker through the same device helper (the bits of tsu_ising3d_energy) and sums the spins alongside.  The
// rest of a ladder does not know the dimension and is the 2-D ladders': the handle's tables and the host side of every entry point
// (pt_host.h), the final sums and q per slot (pt_energy_final, pt_overlap, reduce_dev.h) and the swap pass (pt_dev.h).  This file
// passes in how a half-sweep and an energy partial pass are launched.  No host value changes between rounds: a run of many rounds
// is enqueued without a synchronisation.
#include <cmath>
#include <cstdlib>
#include <new>
#include <vector>

#include "disorder_dev.h"
#include "ising2d.h"
#include "ising3d.h"
#include "corr_dev.h"
#include "pop_host.h"
#include "pt_host.h"
#include "pte_host.h"
#include "reduce_dev.h"

// Parallel tempering: pt_ladder.h's ladder with whole K8 lattices as its walkers, the 3-D counterpart of tsu_pt2d
struct tsu_pt3d : pt_ladder {
    tsu_ising3d** lat;  // walker g = ladder * R + w; lat[0] also holds the one disorder
};

// Population annealing: pop_host.h's population of K8 lattices, all planes in one allocation; `lat` owns the one disorder.  The
// sweeps and the energies are k8_pt_sweep and k8_pt_energy as they stand (every walker at slot 0, the schedule's tables offset by the
// step); the resampling kernels (pop_dev.h) are the 2-D populations' ("Population annealing")
struct tsu_pa3d : pop_handle {
    tsu_ising3d* lat;
};

// Tempering ensemble: pte_host.h's S samples x ladders of K8 lattices, all planes in one allocation and all disorder in another;
// `lat` gives the shape its checks and each sample's disorder its validation ("Tempering ensembles")
struct tsu_pte3d : pte_handle {
    tsu_ising3d* lat;
};

namespace {

struct K8Params {
    int8_t* s;
    const float* jr;     // J_right, J_down, J_layer, h
    const float* jd;
    const float* jl;
    const float* h;
    long long pitch;
    long long nrows;     // depth * rows
    int depth, rows, cols;
    int pz, pr, pc;
    int lshift;          // log2 of the lanes per row
    float c32;           // fl32(2 / T): the screen's scale
    double T;
    uint32_t k0, k1, hs, tag_hi, tag_lo;
};

__device__ __forceinline__ void zero16f(float4* a) {
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// one octet of the colour whose sites sit at chunk positions PAR, PAR + 2, ..
template <int PAR>
__device__ __forceinline__ void k8_octet(const K8Params& p, int z, int r, int q) {
    const long long rho = (long long)z * p.rows + r;
    const long long row = rho * p.pitch;
    const int c0 = 16 * q;
    const bool has_bk = z > 0 || p.pz, has_fw = z + 1 < p.depth || p.pz;
    const bool has_up = r > 0 || p.pr, has_dn = r + 1 < p.rows || p.pr;
    const long long rowb = ((long long)(z > 0 ? z - 1 : p.depth - 1) * p.rows + r) * p.pitch;
    const long long rowf = ((long long)(z + 1 < p.depth ? z + 1 : 0) * p.rows + r) * p.pitch;
    const long long rowu = ((long long)z * p.rows + (r > 0 ? r - 1 : p.rows - 1)) * p.pitch;
    const long long rowd = ((long long)z * p.rows + (r + 1 < p.rows ? r + 1 : 0)) * p.pitch;
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    const uint4 C = *reinterpret_cast<const uint4*>(p.s + row + c0);
    const uint4 B = has_bk ? *reinterpret_cast<const uint4*>(p.s + rowb + c0) : zero4;
    const uint4 F = has_fw ? *reinterpret_cast<const uint4*>(p.s + rowf + c0) : zero4;
    const uint4 U = has_up ? *reinterpret_cast<const uint4*>(p.s + rowu + c0) : zero4;
    const uint4 D = has_dn ? *reinterpret_cast<const uint4*>(p.s + rowd + c0) : zero4;
    float4 jr[4], jd[4], jl[4], ju[4], jb[4], hh[4];
    load16f(p.jr + row + c0, jr);
    load16f(p.jd + row + c0, jd);
    load16f(p.jl + row + c0, jl);
    load16f(p.h + row + c0, hh);
    if (has_up) load16f(p.jd + rowu + c0, ju);
    else zero16f(ju);
    if (has_bk) load16f(p.jl + rowb + c0, jb);
    else zero16f(jb);
    // column c0 - 1 (left of position 0), column c0 + 16 (right of position 15), column 0 (right of the last column, periodic)
    const bool has_prev = q > 0 || p.pc;
    const int cprev = q > 0 ? c0 - 1 : p.cols - 1;
    const int s_prev = has_prev ? (int)p.s[row + cprev] : 0;
    const float j_prev = has_prev ? p.jr[row + cprev] : 0.0f;
    const int s_next = (c0 + 16 < p.cols) ? (int)p.s[row + c0 + 16] : 0;
    const int s_first = p.pc ? (int)p.s[row] : 0;

    const u32x4 w = tsu_philox((uint32_t)q, (uint32_t)rho, p.hs, p.tag_hi, p.k0, p.k1);
    const uint32_t wv[4] = {w.x, w.y, w.z, w.w};
    bool have_lo = false;
    uint32_t lv[4] = {0, 0, 0, 0};
    uint32_t out[4] = {C.x, C.y, C.z, C.w};
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int i = 2 * m + PAR, c = c0 + i;
        if (c >= p.cols) break;
        const bool has_left = i > 0 || has_prev, has_right = c + 1 < p.cols || p.pc;
        const int sb = sbyte(B, i), sf = sbyte(F, i), su = sbyte(U, i), sd = sbyte(D, i);
        const int sl = i > 0 ? sbyte(C, i - 1) : s_prev;
        const int sr = c + 1 < p.cols ? (i < 15 ? sbyte(C, i + 1) : s_next) : s_first;
        const float Jb = has_bk ? fat(jb, i) : 0.0f, Jf = has_fw ? fat(jl, i) : 0.0f;
        const float Ju = has_up ? fat(ju, i) : 0.0f, Jd = has_dn ? fat(jd, i) : 0.0f;
        const float Jl = has_left ? (i > 0 ? fat(jr, i - 1) : j_prev) : 0.0f;
        const float Jr = has_right ? fat(jr, i) : 0.0f;
        const float hf = fat(hh, i);
        // missing neighbours carry J = 0 here: exact in fp32, and the screen only needs a bound (six additions, seven terms)
        const float f32 = (((((Jb * (float)sb + Jf * (float)sf) + Ju * (float)su) + Jd * (float)sd) + Jl * (float)sl) + Jr * (float)sr) + hf;
        const float a32 = fabsf(Jb) + fabsf(Jf) + fabsf(Ju) + fabsf(Jd) + fabsf(Jl) + fabsf(Jr) + fabsf(hf);
        const uint32_t hi = ((wv[m >> 1] >> (16 * (m & 1))) & 0xFFFFu) ^ 0x8000u;
        int dec = screen(f32, a32, p.c32, hi);
        if (dec == 0) {
            // the contract's sum: neighbours in the order z-1, z+1, r-1, r+1, c-1, c+1, a missing one skipped, then h
            double f = 0.0;
            bool any = false;
            if (has_bk) { f = (double)Jb * sb; any = true; }
            if (has_fw) { f = any ? f + (double)Jf * sf : (double)Jf * sf; any = true; }
            if (has_up) { f = any ? f + (double)Ju * su : (double)Ju * su; any = true; }
            if (has_dn) { f = any ? f + (double)Jd * sd : (double)Jd * sd; any = true; }
            if (has_left) { f = any ? f + (double)Jl * sl : (double)Jl * sl; any = true; }
            if (has_right) { f = any ? f + (double)Jr * sr : (double)Jr * sr; any = true; }
            f = any ? f + (double)hf : (double)hf;
            const uint64_t thr = exact_thr(f, p.T);
            const uint32_t thi = (uint32_t)(thr >> 16);
            bool accept = hi < thi;
            if (hi == thi) {  // tie on the top 16 bits: the low half, as K1 draws it
                if (!have_lo) {
                    const u32x4 l = tsu_philox((uint32_t)q, (uint32_t)rho, p.hs, p.tag_lo, p.k0, p.k1);
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

// (row rho, octet q) of a lane: grid (ceil(nrows / (256 >> lshift)), ceil(nchunks / 64)), 256 lanes.  Local row slot j of the
// workgroup's 256 >> lshift rows: the first half of the slots take the even local rows, the second half the odd ones.
template <class P>
__device__ __forceinline__ bool k8_lane(const P& p, long long& rho, int& q) {
    const int t = threadIdx.x;
    const int rpb = 256 >> p.lshift, half = rpb >> 1;
    const int j = t >> p.lshift;
    const int local = j < half ? 2 * j : 2 * (j - half) + 1;
    q = blockIdx.y * 64 + (t & ((1 << p.lshift) - 1));
    rho = (long long)blockIdx.x * rpb + local;
    return rho < p.nrows && 16 * q < p.cols;
}

__global__ __launch_bounds__(256) void k8_sweep(K8Params p, int colour) {
    long long rho;
    int q;
    if (!k8_lane(p, rho, q)) return;
    const int z = (int)(rho / p.rows), r = (int)(rho - (long long)z * p.rows);
    if (((z + r + colour) & 1) == 0) k8_octet<0>(p, z, r, q);
    else k8_octet<1>(p, z, r, q);
}

// i.i.d. +-1: the bits of tsu_ising2d_randomize for a (depth * rows) x cols lattice (global row rho); pad bytes 0
__global__ __launch_bounds__(256) void k8_randomize(K8Params p, uint32_t tag) {
    long long rho;
    int q;
    if (!k8_lane(p, rho, q)) return;
    const u32x4 w = tsu_philox((uint32_t)(q >> 3), (uint32_t)rho, 0u, tag, p.k0, p.k1);
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
            if (16 * q + i >= p.cols) byte = 0;
            v |= byte << (8 * b);
        }
        o[k] = v;
    }
    *reinterpret_cast<uint4*>(p.s + rho * p.pitch + 16 * q) = make_uint4(o[0], o[1], o[2], o[3]);
}

__global__ __launch_bounds__(256) void k8_fill(K8Params p, int value) {
    long long rho;
    int q;
    if (!k8_lane(p, rho, q)) return;
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t byte = (16 * q + 4 * k + b < p.cols) ? (uint32_t)(uint8_t)value : 0u;
            v |= byte << (8 * b);
        }
        o[k] = v;
    }
    *reinterpret_cast<uint4*>(p.s + rho * p.pitch + 16 * q) = make_uint4(o[0], o[1], o[2], o[3]);
}

// E partial of a lane: lane = chunk (rho, q), grid-stride over blockIdx.x in a fixed order; a site adds
// s (((h + J_right s_right) + J_down s_down) + J_layer s_layer), a bond missing on an open axis skipped; ssum = the lane's sum
// of spins.  Shared by the single-lattice and the ladder kernels: the lane order is part of the contract.
__device__ __forceinline__ double k8_energy_lane(const K8Params& p, long long& ssum) {
    const int nchunks = (p.cols + 15) >> 4;
    const long long total = p.nrows * nchunks;
    double e = 0.0;
    long long m = 0;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long rho = t / nchunks;
        const int q = (int)(t - rho * nchunks);
        const int z = (int)(rho / p.rows), r = (int)(rho - (long long)z * p.rows);
        const long long row = rho * p.pitch;
        const bool has_dn = r + 1 < p.rows || p.pr, has_fw = z + 1 < p.depth || p.pz;
        const long long rowd = ((long long)z * p.rows + (r + 1 < p.rows ? r + 1 : 0)) * p.pitch;
        const long long rowf = ((long long)(z + 1 < p.depth ? z + 1 : 0) * p.rows + r) * p.pitch;
        for (int i = 0; i < 16; ++i) {
            const int c = 16 * q + i;
            if (c >= p.cols) break;
            const int s = p.s[row + c];
            double l = (double)p.h[row + c];
            if (c + 1 < p.cols || p.pc) l += (double)p.jr[row + c] * p.s[row + (c + 1 < p.cols ? c + 1 : 0)];
            if (has_dn) l += (double)p.jd[row + c] * p.s[rowd + c];
            if (has_fw) l += (double)p.jl[row + c] * p.s[rowf + c];
            e += s * l;
            m += s;
        }
    }
    ssum = m;
    return e;
}

// E partials: one per workgroup
__global__ __launch_bounds__(256) void k8_energy(K8Params p, double* __restrict__ part) {
    long long m;
    const double e = block_sum(k8_energy_lane(p, m));
    if (threadIdx.x == 0) part[blockIdx.x] = e;
}

// q = sum s^a s^b, one 64-bit vector atomic per workgroup
__global__ __launch_bounds__(256) void k8_overlap(const int8_t* __restrict__ a, const int8_t* __restrict__ b, long long pitch,
                                                  long long nrows, int cols, long long* __restrict__ acc) {
    const long long v = block_isum(pair_lane(a, b, pitch, pitch, nrows, cols));
    if (threadIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long*>(acc), (unsigned long long)v);
}

// sum s
__global__ __launch_bounds__(256) void k8_sum(const int8_t* __restrict__ a, long long pitch, long long nrows, int cols,
                                              long long* __restrict__ acc) {
    const long long v = block_isum(pair_lane(a, nullptr, pitch, pitch, nrows, cols));
    if (threadIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long*>(acc), (unsigned long long)v);
}

// ------------------------------------------------------------------ parallel tempering
struct PT3Params {
    int8_t* const* s;     // walker g = ladder * R + w -> its spins (one pitch for all)
    const uint32_t* key;  // walker -> Philox key (k0, k1) of seed + g
    const int32_t* slot;  // walker -> its slot in its ladder
    const double* T;      // slot -> T
    const float* c32;     // slot -> fl32(2 / T)
    const float* jr;      // the one disorder (K8Params layout)
    const float* jd;
    const float* jl;
    const float* h;
    long long pitch;
    long long nrows;
    int depth, rows, cols;
    int pz, pr, pc;
    int lshift;
    int nw, W;            // walkers; walkers per lane (group z of the grid: walkers [z W, z W + W))
    uint32_t hs;
};

// k8_octet for the walkers [g0, g1): the colour's couplings, fields and the screen's sum of |terms| are staged once, then each
// walker takes the same decision as k8_octet at the temperature of its slot, with its own key (replica 0)
template <int PAR>
__device__ __forceinline__ void k8_pt_octet(const PT3Params& p, int z, int r, int q, int g0, int g1) {
    const long long rho = (long long)z * p.rows + r;
    const long long row = rho * p.pitch;
    const int c0 = 16 * q;
    const bool has_bk = z > 0 || p.pz, has_fw = z + 1 < p.depth || p.pz;
    const bool has_up = r > 0 || p.pr, has_dn = r + 1 < p.rows || p.pr;
    const long long rowb = ((long long)(z > 0 ? z - 1 : p.depth - 1) * p.rows + r) * p.pitch;
    const long long rowf = ((long long)(z + 1 < p.depth ? z + 1 : 0) * p.rows + r) * p.pitch;
    const long long rowu = ((long long)z * p.rows + (r > 0 ? r - 1 : p.rows - 1)) * p.pitch;
    const long long rowd = ((long long)z * p.rows + (r + 1 < p.rows ? r + 1 : 0)) * p.pitch;
    const bool has_prev = q > 0 || p.pc;
    const int cprev = q > 0 ? c0 - 1 : p.cols - 1;
    // the colour's 8 sites: J to the six neighbours (0 where one is missing), h, and the screen's sum of |terms|
    float Jb[8], Jf[8], Ju[8], Jd[8], Jl[8], Jr[8], hf[8], a32[8];
    {
        float4 jr[4], jd[4], jl[4], ju[4], jb[4], hh[4];
        load16f(p.jr + row + c0, jr);
        load16f(p.jd + row + c0, jd);
        load16f(p.jl + row + c0, jl);
        load16f(p.h + row + c0, hh);
        if (has_up) load16f(p.jd + rowu + c0, ju);
        else zero16f(ju);
        if (has_bk) load16f(p.jl + rowb + c0, jb);
        else zero16f(jb);
        const float j_prev = has_prev ? p.jr[row + cprev] : 0.0f;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int i = 2 * m + PAR, c = c0 + i;
            const bool has_left = i > 0 || has_prev, has_right = c + 1 < p.cols || p.pc;
            Jb[m] = has_bk ? fat(jb, i) : 0.0f;
            Jf[m] = has_fw ? fat(jl, i) : 0.0f;
            Ju[m] = has_up ? fat(ju, i) : 0.0f;
            Jd[m] = has_dn ? fat(jd, i) : 0.0f;
            Jl[m] = has_left ? (i > 0 ? fat(jr, i - 1) : j_prev) : 0.0f;
            Jr[m] = has_right ? fat(jr, i) : 0.0f;
            hf[m] = fat(hh, i);
            a32[m] = fabsf(Jb[m]) + fabsf(Jf[m]) + fabsf(Ju[m]) + fabsf(Jd[m]) + fabsf(Jl[m]) + fabsf(Jr[m]) + fabsf(hf[m]);
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
        const uint4 B = has_bk ? *reinterpret_cast<const uint4*>(s + rowb + c0) : zero4;
        const uint4 F = has_fw ? *reinterpret_cast<const uint4*>(s + rowf + c0) : zero4;
        const uint4 U = has_up ? *reinterpret_cast<const uint4*>(s + rowu + c0) : zero4;
        const uint4 D = has_dn ? *reinterpret_cast<const uint4*>(s + rowd + c0) : zero4;
        const int s_prev = has_prev ? (int)s[row + cprev] : 0;
        const int s_next = (c0 + 16 < p.cols) ? (int)s[row + c0 + 16] : 0;
        const int s_first = p.pc ? (int)s[row] : 0;
        const u32x4 w = tsu_philox((uint32_t)q, (uint32_t)rho, p.hs, TSU_TAG_ISING_HI, k0, k1);
        const uint32_t wv[4] = {w.x, w.y, w.z, w.w};
        bool have_lo = false;
        uint32_t lv[4] = {0, 0, 0, 0};
        uint32_t out[4] = {C.x, C.y, C.z, C.w};
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int i = 2 * m + PAR, c = c0 + i;
            if (c >= p.cols) break;
            const bool has_left = i > 0 || has_prev, has_right = c + 1 < p.cols || p.pc;
            const int sb = sbyte(B, i), sf = sbyte(F, i), su = sbyte(U, i), sd = sbyte(D, i);
            const int sl = i > 0 ? sbyte(C, i - 1) : s_prev;
            const int sr = c + 1 < p.cols ? (i < 15 ? sbyte(C, i + 1) : s_next) : s_first;
            const float f32 =
                (((((Jb[m] * (float)sb + Jf[m] * (float)sf) + Ju[m] * (float)su) + Jd[m] * (float)sd) + Jl[m] * (float)sl) + Jr[m] * (float)sr) +
                hf[m];
            const uint32_t hi = ((wv[m >> 1] >> (16 * (m & 1))) & 0xFFFFu) ^ 0x8000u;
            int dec = screen(f32, a32[m], c32, hi);
            if (dec == 0) {
                // the contract's sum: neighbours in the order z-1, z+1, r-1, r+1, c-1, c+1, a missing one skipped, then h
                double f = 0.0;
                bool any = false;
                if (has_bk) { f = (double)Jb[m] * sb; any = true; }
                if (has_fw) { f = any ? f + (double)Jf[m] * sf : (double)Jf[m] * sf; any = true; }
                if (has_up) { f = any ? f + (double)Ju[m] * su : (double)Ju[m] * su; any = true; }
                if (has_dn) { f = any ? f + (double)Jd[m] * sd : (double)Jd[m] * sd; any = true; }
                if (has_left) { f = any ? f + (double)Jl[m] * sl : (double)Jl[m] * sl; any = true; }
                if (has_right) { f = any ? f + (double)Jr[m] * sr : (double)Jr[m] * sr; any = true; }
                f = any ? f + (double)hf[m] : (double)hf[m];
                const uint64_t thr = exact_thr(f, T);
                const uint32_t thi = (uint32_t)(thr >> 16);
                bool accept = hi < thi;
                if (hi == thi) {  // tie on the top 16 bits: the low half, as K1 draws it
                    if (!have_lo) {
                        const u32x4 l = tsu_philox((uint32_t)q, (uint32_t)rho, p.hs, TSU_TAG_ISING_LO, k0, k1);
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

// k8_sweep's grid with the walker group as its z dimension: lane = octet q of row rho (k8_lane) for the walkers of group z.
// The 64 staged floats and five spin vectors fit 255 VGPRs without scratch; the second launch bound keeps the allocator from
// spreading into AGPRs, which would halve the waves per SIMD for nothing.
__global__ __launch_bounds__(256, 2) void k8_pt_sweep(PT3Params p, int colour) {
    long long rho;
    int q;
    if (!k8_lane(p, rho, q)) return;
    const int z = (int)(rho / p.rows), r = (int)(rho - (long long)z * p.rows);
    const int g0 = blockIdx.z * p.W, g1 = min(g0 + p.W, p.nw);
    if (((z + r + colour) & 1) == 0) k8_pt_octet<0>(p, z, r, q, g0, g1);
    else k8_pt_octet<1>(p, z, r, q, g0, g1);
}

// The ensemble's sample index: grid z of the sweep = sample * groups + walker group, walkers [base + group W, ..) clipped to the
// sample's own [base, base + nper), base = sample * nper; the sample's disorder sits dstride floats after its predecessor's
struct PTEns {
    long long dstride;  // floats of a sample's disorder (4 planes)
    int nper;           // walkers of a sample (nl * R)
    int groups;         // walker groups of a sample: ceil(nper / W)
};

__device__ __forceinline__ void pte_sample(PT3Params& p, const PTEns& e, int sample) {
    const long long off = (long long)sample * e.dstride;
    p.jr += off;
    p.jd += off;
    p.jl += off;
    p.h += off;
}

// k8_pt_sweep for an ensemble, a kernel of its own so that the ladders' code object stays what it was: the same lane and the same
// octet, for the walkers of one group of one sample on that sample's disorder.  The sample and its offsets are wave-uniform.
__global__ __launch_bounds__(256, 2) void k8_pte_sweep(PT3Params p, PTEns e, int colour) {
    long long rho;
    int q;
    if (!k8_lane(p, rho, q)) return;
    const int z = (int)(rho / p.rows), r = (int)(rho - (long long)z * p.rows);
    const int sample = blockIdx.z / e.groups, group = blockIdx.z - sample * e.groups;
    const int base = sample * e.nper;
    const int g0 = base + group * p.W, g1 = min(g0 + p.W, base + e.nper);
    pte_sample(p, e, sample);
    if (((z + r + colour) & 1) == 0) k8_pt_octet<0>(p, z, r, q, g0, g1);
    else k8_pt_octet<1>(p, z, r, q, g0, g1);
}

__device__ __forceinline__ K8Params pt_walker_params(const PT3Params& pp, int g) {
    K8Params p;
    p.s = pp.s[g];
    p.jr = pp.jr;
    p.jd = pp.jd;
    p.jl = pp.jl;
    p.h = pp.h;
    p.pitch = pp.pitch;
    p.nrows = pp.nrows;
    p.depth = pp.depth;
    p.rows = pp.rows;
    p.cols = pp.cols;
    p.pz = pp.pz;
    p.pr = pp.pr;
    p.pc = pp.pc;
    p.lshift = pp.lshift;
    p.c32 = 0.0f;
    p.T = 0.0;
    p.k0 = p.k1 = p.hs = p.tag_hi = p.tag_lo = 0;
    return p;
}

// grid (blocks_for(lattice), nw): workgroup x of walker y computes k8_energy's partial x of that walker alone, and its sum of spins
__global__ __launch_bounds__(256) void k8_pt_energy(PT3Params pp, double* __restrict__ part, long long* __restrict__ ipart) {
    long long m;
    const double e = block_sum(k8_energy_lane(pt_walker_params(pp, blockIdx.y), m));
    const long long ms = block_isum(m);
    if (threadIdx.x == 0) {
        part[(size_t)blockIdx.y * kEnergyBlocks + blockIdx.x] = e;
        ipart[(size_t)blockIdx.y * kEnergyBlocks + blockIdx.x] = ms;
    }
}

// k8_pt_energy for an ensemble: walker y on the disorder of its sample y / nper
__global__ __launch_bounds__(256) void k8_pte_energy(PT3Params pp, PTEns en, double* __restrict__ part, long long* __restrict__ ipart) {
    pte_sample(pp, en, blockIdx.y / en.nper);
    long long m;
    const double e = block_sum(k8_energy_lane(pt_walker_params(pp, blockIdx.y), m));
    const long long ms = block_isum(m);
    if (threadIdx.x == 0) {
        part[(size_t)blockIdx.y * kEnergyBlocks + blockIdx.x] = e;
        ipart[(size_t)blockIdx.y * kEnergyBlocks + blockIdx.x] = ms;
    }
}

K8Params make_params(const tsu_ising3d* L) {
    K8Params p;
    const size_t plane = (size_t)L->depth * L->rows * L->pitch;
    p.s = L->s;
    p.jr = L->d_dis;
    p.jd = L->d_dis ? L->d_dis + plane : nullptr;
    p.jl = L->d_dis ? L->d_dis + 2 * plane : nullptr;
    p.h = L->d_dis ? L->d_dis + 3 * plane : nullptr;
    p.pitch = (long long)L->pitch;
    p.nrows = (long long)L->depth * L->rows;
    p.depth = L->depth;
    p.rows = L->rows;
    p.cols = L->cols;
    p.pz = L->pz;
    p.pr = L->pr;
    p.pc = L->pc;
    const int nchunks = (L->cols + 15) >> 4;
    p.lshift = 0;
    while (p.lshift < 6 && (1 << p.lshift) < nchunks) ++p.lshift;
    p.c32 = 0.0f;
    p.T = 0.0;
    p.k0 = p.k1 = p.hs = p.tag_hi = p.tag_lo = 0;
    return p;
}

// grid of the lane-per-octet kernels (k8_lane)
dim3 octet_grid(const K8Params& p) {
    const long long rpb = 256 >> p.lshift;
    const int nchunks = (p.cols + 15) >> 4;
    return dim3((unsigned)((p.nrows + rpb - 1) / rpb), (unsigned)((nchunks + 63) / 64), 1);
}

unsigned blocks_for(const tsu_ising3d* L) { return reduce_blocks((long long)L->depth * L->rows * ((L->cols + 15) / 16)); }

int read_acc(tsu_ising3d* L, int64_t* out) {
    tsu_ctx* ctx = L->ctx;
    TSU_HIP_TRY(ctx, hipGetLastError());
    int64_t h = 0;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(&h, L->d_acc, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *out = h;
    return ising3d_check_err(L);
}

void pt_free(tsu_pt3d* P) { pt_delete(P, tsu_ising3d_destroy); }

PT3Params pt_params(const tsu_pt3d* P) {
    const K8Params k = make_params(P->lat[0]);
    PT3Params p;
    p.s = P->d_s;
    p.key = P->d_key;
    p.slot = P->d_slot;
    p.T = P->d_T;
    p.c32 = P->d_c32;
    p.jr = k.jr;
    p.jd = k.jd;
    p.jl = k.jl;
    p.h = k.h;
    p.pitch = k.pitch;
    p.nrows = k.nrows;
    p.depth = k.depth;
    p.rows = k.rows;
    p.cols = k.cols;
    p.pz = k.pz;
    p.pr = k.pr;
    p.pc = k.pc;
    p.lshift = k.lshift;
    p.nw = P->nw;
    p.W = 1;
    p.hs = 0;
    return p;
}

// k8_pt_energy into d_part / d_ipart (asynchronous): the partial pass pt_host.h's energies take
auto pt_partials(tsu_pt3d* P, const PT3Params& p) {
    return [P, &p](unsigned blocks) { k8_pt_energy<<<dim3(blocks, (unsigned)P->nw, 1), 256, 0, P->ctx->stream>>>(p, P->d_part, P->d_ipart); };
}

void pte_free(tsu_pte3d* P) { pte_delete(P, tsu_ising3d_destroy); }

// the ladders' parameters for an ensemble: sample 0's disorder (the kernels add the sample's offset), the walkers of all samples
PT3Params pte_params(const tsu_pte3d* P) {
    const K8Params k = make_params(P->lat);
    PT3Params p;
    p.s = P->d_s;
    p.key = P->d_key;
    p.slot = P->d_slot;
    p.T = P->d_T;
    p.c32 = P->d_c32;
    p.jr = P->d_dis;
    p.jd = P->d_dis + P->plane;
    p.jl = P->d_dis + 2 * P->plane;
    p.h = P->d_dis + 3 * P->plane;
    p.pitch = k.pitch;
    p.nrows = k.nrows;
    p.depth = k.depth;
    p.rows = k.rows;
    p.cols = k.cols;
    p.pz = k.pz;
    p.pr = k.pr;
    p.pc = k.pc;
    p.lshift = k.lshift;
    p.nw = P->nw;
    p.W = 1;
    p.hs = 0;
    return p;
}

PTEns pte_ens(const tsu_pte3d* P, int W) {
    PTEns e;
    e.dstride = 4 * (long long)P->plane;
    e.nper = P->nl * P->R;
    e.groups = (int)pte_groups(P, W);
    return e;
}

// k8_pte_energy into d_part / d_ipart (asynchronous)
auto pte_partials(tsu_pte3d* P, const PT3Params& p, const PTEns& e) {
    return [P, &p, &e](unsigned blocks) {
        k8_pte_energy<<<dim3(blocks, (unsigned)P->nw, 1), 256, 0, P->ctx->stream>>>(p, e, P->d_part, P->d_ipart);
    };
}

void pa_free(tsu_pa3d* P) { pop_delete(P, tsu_ising3d_destroy); }

// the ladders' parameters for a population: walker -> plane, key and slot 0; T / c32 are set per step
PT3Params pa_params(const tsu_pa3d* P) {
    const K8Params k = make_params(P->lat);
    PT3Params p;
    p.s = P->d_s;
    p.key = P->d_key;
    p.slot = P->d_slot;
    p.T = P->d_T;
    p.c32 = P->d_c32;
    p.jr = k.jr;
    p.jd = k.jd;
    p.jl = k.jl;
    p.h = k.h;
    p.pitch = k.pitch;
    p.nrows = k.nrows;
    p.depth = k.depth;
    p.rows = k.rows;
    p.cols = k.cols;
    p.pz = k.pz;
    p.pr = k.pr;
    p.pc = k.pc;
    p.lshift = k.lshift;
    p.nw = P->R;
    p.W = pop_group(P);
    p.hs = 0;
    return p;
}

// half-sweep hs of every walker at step k's temperature / the energy partial pass: what pop_host.h's init and run take
auto pa_sweep(tsu_pa3d* P, PT3Params& p) {
    const dim3 og = octet_grid(make_params(P->lat));
    const dim3 grid(og.x, og.y, (unsigned)((P->R + p.W - 1) / p.W));
    return [P, &p, grid](uint32_t hs, int colour, int k) {
        p.hs = hs;
        p.T = P->d_T + k;
        p.c32 = P->d_c32 + k;
        k8_pt_sweep<<<grid, 256, 0, P->ctx->stream>>>(p, colour);
    };
}

auto pa_partials(tsu_pa3d* P, const PT3Params& p) {
    return [P, &p](unsigned blocks) { k8_pt_energy<<<dim3(blocks, (unsigned)P->R, 1), 256, 0, P->ctx->stream>>>(p, P->d_part, P->d_ipart); };
}

}  // namespace

extern "C" {

int tsu_ising3d_create(tsu_ctx* ctx, int depth, int rows, int cols, int periodic_mask, tsu_ising3d** out) {
    TSU_ENTER(ctx);
    if (!ctx || !out) return TSU_E_INVALID;
    *out = nullptr;
    TSU_REQUIRE(ctx, depth >= 1 && rows >= 1 && cols >= 1, "ising3d: depth/rows/cols must be positive");
    TSU_REQUIRE(ctx, (periodic_mask & ~7) == 0, "ising3d: periodic_mask must be a combination of TSU_PERIODIC_Z / _R / _C, got %d",
                periodic_mask);
    TSU_REQUIRE(ctx, (long long)depth * rows < (1ll << 31) && cols <= (1 << 30), "ising3d: lattice too large for 32-bit counters");
    const int len[3] = {depth, rows, cols};
    const char* axis[3] = {"depth", "rows", "cols"};
    for (int a = 0; a < 3; ++a)
        if (((periodic_mask >> a) & 1) && ((len[a] & 1) || len[a] < 4))
            return tsu_fail(ctx, TSU_E_UNSUPPORTED, "ising3d: a periodic axis needs an even length >= 4 (%s = %d)", axis[a], len[a]);
    tsu_ising3d* L = new (std::nothrow) tsu_ising3d();
    if (!L) return tsu_fail(ctx, TSU_E_NOMEM, "ising3d: host allocation failed");
    L->ctx = ctx;
    L->depth = depth;
    L->rows = rows;
    L->cols = cols;
    L->pz = (periodic_mask >> 0) & 1;
    L->pr = (periodic_mask >> 1) & 1;
    L->pc = (periodic_mask >> 2) & 1;
    L->pitch = ((size_t)cols + 15) / 16 * 16;
    const size_t bytes = (size_t)depth * rows * L->pitch;
    hipError_t e = hipMalloc((void**)&L->s, bytes);
    if (e == hipSuccess) e = hipMemsetAsync(L->s, 0, bytes, ctx->stream);
    if (e == hipSuccess) e = hipMalloc((void**)&L->d_part, (kEnergyBlocks + 1) * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&L->d_acc, sizeof(long long));
    if (e != hipSuccess) {
        const int rc = tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "ising3d_create: %s (%zu bytes)",
                                hipGetErrorString(e), bytes);
        if (L->s) (void)hipFree(L->s);
        if (L->d_part) (void)hipFree(L->d_part);
        if (L->d_acc) (void)hipFree(L->d_acc);
        delete L;
        return rc;
    }
    *out = L;
    return TSU_OK;
}

int tsu_ising3d_destroy(tsu_ising3d* L) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_OK;
    (void)hipStreamSynchronize(L->ctx->stream);
    if (L->s) (void)hipFree(L->s);
    if (L->d_dis) (void)hipFree(L->d_dis);
    if (L->d_part) (void)hipFree(L->d_part);
    if (L->d_acc) (void)hipFree(L->d_acc);
    if (L->d_prof) (void)hipFree(L->d_prof);
    ising3d_cluster_free(L);
    delete L;
    return TSU_OK;
}

int tsu_ising3d_set_spins(tsu_ising3d* L, const int8_t* host) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, host, "ising3d_set_spins: NULL input");
    TSU_HIP_TRY(ctx, hipMemcpy2DAsync(L->s, L->pitch, host, (size_t)L->cols, (size_t)L->cols, (size_t)L->depth * L->rows,
                                      hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int tsu_ising3d_get_spins(tsu_ising3d* L, int8_t* host) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, host, "ising3d_get_spins: NULL output");
    TSU_HIP_TRY(ctx, hipMemcpy2DAsync(host, (size_t)L->cols, L->s, L->pitch, (size_t)L->cols, (size_t)L->depth * L->rows,
                                      hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ising3d_check_err(L);
}

int tsu_ising3d_randomize(tsu_ising3d* L, uint64_t seed, uint32_t replica) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    K8Params p = make_params(L);
    p.k0 = (uint32_t)seed;
    p.k1 = (uint32_t)(seed >> 32);
    k8_randomize<<<octet_grid(p), 256, 0, ctx->stream>>>(p, TSU_TAG_INIT | (replica << 8));
    TSU_HIP_TRY(ctx, hipGetLastError());
    return TSU_OK;
}

int tsu_ising3d_fill(tsu_ising3d* L, int8_t value) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, value == 1 || value == -1, "ising3d_fill: value must be +1 or -1");
    const K8Params p = make_params(L);
    k8_fill<<<octet_grid(p), 256, 0, ctx->stream>>>(p, (int)value);
    TSU_HIP_TRY(ctx, hipGetLastError());
    return TSU_OK;
}

int tsu_ising3d_set_disorder(tsu_ising3d* L, const float* J_right, const float* J_down, const float* J_layer, const float* h) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, J_right && J_down && J_layer, "ising3d_set_disorder: J_right, J_down and J_layer are required (h may be NULL)");
    const int depth = L->depth, rows = L->rows, cols = L->cols;
    for (int z = 0; z < depth; ++z)
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) {
                const size_t i = ((size_t)z * rows + r) * cols + c;
                TSU_REQUIRE(ctx, std::isfinite(J_right[i]) && std::isfinite(J_down[i]) && std::isfinite(J_layer[i]) && (!h || std::isfinite(h[i])),
                            "ising3d_set_disorder: non-finite value at site (%d, %d, %d)", z, r, c);
                TSU_REQUIRE(ctx, L->pc || c + 1 < cols || J_right[i] == 0.0f,
                            "ising3d_set_disorder: open axis: J_right[%d, %d, %d] (last column) must be 0, got %g", z, r, c, (double)J_right[i]);
                TSU_REQUIRE(ctx, L->pr || r + 1 < rows || J_down[i] == 0.0f,
                            "ising3d_set_disorder: open axis: J_down[%d, %d, %d] (last row) must be 0, got %g", z, r, c, (double)J_down[i]);
                TSU_REQUIRE(ctx, L->pz || z + 1 < depth || J_layer[i] == 0.0f,
                            "ising3d_set_disorder: open axis: J_layer[%d, %d, %d] (last layer) must be 0, got %g", z, r, c, (double)J_layer[i]);
            }
    int have_field = 0;
    if (h)
        for (size_t i = 0, n = (size_t)depth * rows * cols; i < n && !have_field; ++i) have_field = h[i] != 0.0f;
    const size_t nrows = (size_t)depth * rows, plane = nrows * L->pitch;
    if (!L->d_dis) {
        TSU_HIP_TRY(ctx, hipMalloc((void**)&L->d_dis, 4 * plane * sizeof(float)));
        TSU_HIP_TRY(ctx, hipMemsetAsync(L->d_dis, 0, 4 * plane * sizeof(float), ctx->stream));  // pad columns stay 0
    }
    const size_t dpitch = L->pitch * sizeof(float), w = (size_t)cols * sizeof(float);
    const float* src[3] = {J_right, J_down, J_layer};
    for (int k = 0; k < 3; ++k)
        TSU_HIP_TRY(ctx, hipMemcpy2DAsync(L->d_dis + k * plane, dpitch, src[k], w, w, nrows, hipMemcpyHostToDevice, ctx->stream));
    if (h) TSU_HIP_TRY(ctx, hipMemcpy2DAsync(L->d_dis + 3 * plane, dpitch, h, w, w, nrows, hipMemcpyHostToDevice, ctx->stream));
    else TSU_HIP_TRY(ctx, hipMemsetAsync(L->d_dis + 3 * plane, 0, plane * sizeof(float), ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    L->have_disorder = 1;
    L->have_field = have_field;
    return TSU_OK;
}

int tsu_ising3d_sweep(tsu_ising3d* L, double T, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, L->have_disorder, "ising3d_sweep: call tsu_ising3d_set_disorder first");
    TSU_REQUIRE(ctx, T > 0.0 && std::isfinite(T), "Temperature must be positive");
    TSU_REQUIRE(ctx, n_sweeps >= 0, "ising3d_sweep: n_sweeps must be >= 0");
    TSU_REQUIRE(ctx, (uint64_t)sweep0 + (uint64_t)n_sweeps <= (1ull << 31), "ising3d_sweep: sweep counter overflow");
    if (n_sweeps == 0) return TSU_OK;
    K8Params p = make_params(L);
    ising2d_set_keys(p, seed, replica);
    p.T = T;
    p.c32 = (float)(2.0 / T);
    const dim3 grid = octet_grid(p);
    for (int s = 0; s < n_sweeps; ++s)
        for (int colour = 0; colour < 2; ++colour) {
            p.hs = 2u * (sweep0 + (uint32_t)s) + (uint32_t)colour;
            k8_sweep<<<grid, 256, 0, ctx->stream>>>(p, colour);
            L->launches += 1;
        }
    TSU_HIP_TRY(ctx, hipGetLastError());
    return TSU_OK;
}

int tsu_ising3d_energy(tsu_ising3d* L, double* E) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, E, "ising3d_energy: NULL output");
    TSU_REQUIRE(ctx, L->have_disorder, "ising3d_energy: call tsu_ising3d_set_disorder first");
    const unsigned blocks = blocks_for(L);
    const K8Params p = make_params(L);
    k8_energy<<<blocks, 256, 0, ctx->stream>>>(p, L->d_part);
    energy_final<<<1, 256, 0, ctx->stream>>>(L->d_part, (int)blocks, L->d_part + kEnergyBlocks);
    TSU_HIP_TRY(ctx, hipGetLastError());
    double e = 0.0;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(&e, L->d_part + kEnergyBlocks, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *E = e;
    return ising3d_check_err(L);
}

int tsu_ising3d_sum_spins(tsu_ising3d* L, int64_t* sum_s) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, sum_s, "ising3d_sum_spins: NULL output");
    TSU_HIP_TRY(ctx, hipMemsetAsync(L->d_acc, 0, sizeof(long long), ctx->stream));
    k8_sum<<<blocks_for(L), 256, 0, ctx->stream>>>(L->s, (long long)L->pitch, (long long)L->depth * L->rows, L->cols, L->d_acc);
    return read_acc(L, sum_s);
}

int tsu_ising3d_overlap(tsu_ising3d* A, tsu_ising3d* B, int64_t* q) {
    TSU_ENTER(A ? A->ctx : nullptr);
    if (!A || !B) return TSU_E_INVALID;
    tsu_ctx* ctx = A->ctx;
    TSU_REQUIRE(ctx, q, "ising3d_overlap: NULL output");
    TSU_REQUIRE(ctx, B->ctx == ctx, "ising3d_overlap: the two lattices belong to different contexts");
    TSU_REQUIRE(ctx, A->depth == B->depth && A->rows == B->rows && A->cols == B->cols,
                "ising3d_overlap: shapes differ (%d x %d x %d against %d x %d x %d)", A->depth, A->rows, A->cols, B->depth, B->rows, B->cols);
    TSU_HIP_TRY(ctx, hipMemsetAsync(A->d_acc, 0, sizeof(long long), ctx->stream));
    k8_overlap<<<blocks_for(A), 256, 0, ctx->stream>>>(A->s, B->s, (long long)A->pitch, (long long)A->depth * A->rows, A->cols, A->d_acc);
    return read_acc(A, q);
}

int tsu_ising3d_link_overlap(tsu_ising3d* A, tsu_ising3d* B, int64_t* Lout, int64_t* n_bonds) {
    TSU_ENTER(A ? A->ctx : nullptr);
    if (!A || !B) return TSU_E_INVALID;
    tsu_ctx* ctx = A->ctx;
    TSU_REQUIRE(ctx, Lout && n_bonds, "ising3d_link_overlap: NULL output");
    TSU_REQUIRE(ctx, B->ctx == ctx, "ising3d_link_overlap: the two lattices belong to different contexts");
    TSU_REQUIRE(ctx, A->depth == B->depth && A->rows == B->rows && A->cols == B->cols,
                "ising3d_link_overlap: shapes differ (%d x %d x %d against %d x %d x %d)", A->depth, A->rows, A->cols, B->depth, B->rows,
                B->cols);
    TSU_REQUIRE(ctx, A->pz == B->pz && A->pr == B->pr && A->pc == B->pc, "ising3d_link_overlap: the periodic axes of the two lattices differ");
    LinkArgs la;
    const unsigned blocks = link_plan(la, (long long)A->pitch, (long long)B->pitch, (long long)A->depth * A->rows, A->rows, A->cols, A->pz, A->pr, A->pc);
    TSU_HIP_TRY(ctx, hipMemsetAsync(A->d_acc, 0, sizeof(long long), ctx->stream));
    link_pass<<<blocks, 256, 0, ctx->stream>>>(A->s, B->s, la, A->d_acc);
    *n_bonds = link_bonds(A->depth, A->rows, A->cols, A->pz, A->pr, A->pc);
    return read_acc(A, Lout);
}

int tsu_ising3d_profiles(tsu_ising3d* A, tsu_ising3d* B, int64_t* p_z, int64_t* p_r, int64_t* p_c) {
    TSU_ENTER(A ? A->ctx : nullptr);
    if (!A) return TSU_E_INVALID;
    tsu_ctx* ctx = A->ctx;
    TSU_REQUIRE(ctx, p_z && p_r && p_c, "ising3d_profiles: NULL output");
    if (B) {
        TSU_REQUIRE(ctx, B->ctx == ctx, "ising3d_profiles: the two lattices belong to different contexts");
        TSU_REQUIRE(ctx, A->depth == B->depth && A->rows == B->rows && A->cols == B->cols,
                    "ising3d_profiles: shapes differ (%d x %d x %d against %d x %d x %d)", A->depth, A->rows, A->cols, B->depth, B->rows,
                    B->cols);
    }
    const size_t n = (size_t)A->depth + (size_t)A->rows + (size_t)A->cols;
    if (!A->d_prof) TSU_HIP_TRY(ctx, hipMalloc((void**)&A->d_prof, n * sizeof(long long)));
    TSU_HIP_TRY(ctx, hipMemsetAsync(A->d_prof, 0, n * sizeof(long long), ctx->stream));
    ProfArgs pa;
    const dim3 grid = profile_plan(pa, (long long)A->pitch, B ? (long long)B->pitch : 0, (long long)A->depth * A->rows, A->rows, A->cols, 1, 1);
    profile_pass<<<grid, 256, 0, ctx->stream>>>(A->s, B ? B->s : nullptr, pa, A->d_prof);
    TSU_HIP_TRY(ctx, hipGetLastError());
    int64_t* out[3] = {p_z, p_r, p_c};
    const int len[3] = {A->depth, A->rows, A->cols};
    const long long* src = A->d_prof;
    for (int a = 0; a < 3; ++a) {
        TSU_HIP_TRY(ctx, hipMemcpyAsync(out[a], src, (size_t)len[a] * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        src += len[a];
    }
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ising3d_check_err(A);
}

int tsu_ising3d_launch_count(tsu_ising3d* L, uint64_t* n) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L || !n) return TSU_E_INVALID;
    *n = L->launches;
    return TSU_OK;
}

// ------------------------------------------------------------------ parallel tempering
int tsu_pt3d_create(tsu_ctx* ctx, int depth, int rows, int cols, int periodic_mask, int n_temps, int n_ladders, tsu_pt3d** out) {
    TSU_ENTER(ctx);
    if (!ctx || !out) return TSU_E_INVALID;
    return pt_create(
        ctx, "pt3d", n_temps, n_ladders, out,
        [=](tsu_ising3d** L) { return tsu_ising3d_create(ctx, depth, rows, cols, periodic_mask, L); },
        [](tsu_pt3d* P, int8_t** planes) {
            P->nrows = (long long)P->lat[0]->depth * P->lat[0]->rows;
            P->pitch = (long long)P->lat[0]->pitch;
            P->cols = P->lat[0]->cols;
            P->n_axes = 3;
            P->lrows = P->lat[0]->rows;
            P->axis_len[0] = P->lat[0]->depth;
            P->axis_len[1] = P->lat[0]->rows;
            P->axis_len[2] = P->lat[0]->cols;
            P->axis_per[0] = P->lat[0]->pz;
            P->axis_per[1] = P->lat[0]->pr;
            P->axis_per[2] = P->lat[0]->pc;
            for (int g = 0; g < P->nw; ++g) planes[g] = P->lat[g]->s;
        },
        pt_free);
}

int tsu_pt3d_destroy(tsu_pt3d* P) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_OK;
    (void)hipStreamSynchronize(P->ctx->stream);
    pt_free(P);
    return TSU_OK;
}

int tsu_pt3d_set_disorder(tsu_pt3d* P, const float* J_right, const float* J_down, const float* J_layer, const float* h) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    return tsu_ising3d_set_disorder(P->lat[0], J_right, J_down, J_layer, h);  // stored once, with walker 0's lattice
}

int tsu_pt3d_set_temperatures(tsu_pt3d* P, const double* T) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_set_temperatures(P, T) : TSU_E_INVALID;
}

int tsu_pt3d_init(tsu_pt3d* P, uint64_t seed, int initial) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    return pt_init(
        P, seed, initial,
        [=](int g, uint64_t s) {  // temperature_scan_3d's model g
            return initial == 0 ? tsu_ising3d_randomize(P->lat[g], s, 0) : tsu_ising3d_fill(P->lat[g], (int8_t)initial);
        },
        [] { return (int)TSU_OK; });
}

int tsu_pt3d_run(tsu_pt3d* P, int n_rounds, int swap_interval, int do_swap, int record) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    tsu_ising3d* L = P->lat[0];
    const int rc = pt_run_check(P, L->have_disorder, n_rounds, swap_interval);
    if (rc != TSU_OK) return rc;
    PT3Params p = pt_params(P);
    p.W = pt_group(P);
    const dim3 og = octet_grid(make_params(L));
    const dim3 grid(og.x, og.y, (unsigned)((P->nw + p.W - 1) / p.W));
    return pt_run(
        P, n_rounds, swap_interval, do_swap, record,
        [&](uint32_t hs, int colour) {
            p.hs = hs;
            k8_pt_sweep<<<grid, 256, 0, ctx->stream>>>(p, colour);
        },
        pt_partials(P, p), [] { return (int)TSU_OK; });
}

int tsu_pt3d_history(tsu_pt3d* P, double* E, int64_t* M, int64_t* q, int32_t* walker) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_history(P, E, M, q, walker) : TSU_E_INVALID;
}

int tsu_pt3d_stats(tsu_pt3d* P, int64_t* attempts, int64_t* accepts, int64_t* round_trips, int32_t* walker_at_slot, uint64_t* sweep_count,
                   uint64_t* round_count) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_stats(P, attempts, accepts, round_trips, walker_at_slot, sweep_count, round_count) : TSU_E_INVALID;
}

int tsu_pt3d_energies(tsu_pt3d* P, double* E, int64_t* sum_s) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const PT3Params p = pt_params(P);
    return pt_energies(P, P->lat[0]->have_disorder, E, sum_s, pt_partials(P, p));
}

int tsu_pt3d_get_spins(tsu_pt3d* P, int ladder, int slot, int8_t* host) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    TSU_REQUIRE(P->ctx, host, "pt3d_get_spins: NULL output");
    int g = 0;
    const int rc = pt_at(P, ladder, slot, "get_spins", &g);
    return rc != TSU_OK ? rc : tsu_ising3d_get_spins(P->lat[g], host);
}

int tsu_pt3d_set_spins(tsu_pt3d* P, int ladder, int slot, const int8_t* host) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    TSU_REQUIRE(P->ctx, host, "pt3d_set_spins: NULL input");
    int g = 0;
    const int rc = pt_at(P, ladder, slot, "set_spins", &g);
    return rc != TSU_OK ? rc : tsu_ising3d_set_spins(P->lat[g], host);
}

int tsu_pt3d_launch_count(tsu_pt3d* P, uint64_t* n) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return pt_launch_count(P, n);
}

int tsu_pt3d_set_correlation(tsu_pt3d* P, int enable, const double* cos_z, const double* sin_z, const double* cos_r, const double* sin_r,
                             const double* cos_c, const double* sin_c) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const double* cs[3] = {cos_z, cos_r, cos_c};
    const double* sn[3] = {sin_z, sin_r, sin_c};
    return pt_set_correlation(P, enable, cs, sn);
}

int tsu_pt3d_history_modes(tsu_pt3d* P, double* modes) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_history_modes(P, modes) : TSU_E_INVALID;
}

int tsu_pt3d_profiles(tsu_pt3d* P, int slot, int64_t* p_z, int64_t* p_r, int64_t* p_c) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    int64_t* out[3] = {p_z, p_r, p_c};
    return pt_profiles(P, slot, out);
}

int tsu_pt3d_set_link_overlap(tsu_pt3d* P, int enable) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_set_link_overlap(P, enable) : TSU_E_INVALID;
}

int tsu_pt3d_history_link(tsu_pt3d* P, int64_t* L) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_history_link(P, L) : TSU_E_INVALID;
}

// ------------------------------------------------------------------ tempering ensembles
int tsu_pte3d_create(tsu_ctx* ctx, int depth, int rows, int cols, int periodic_mask, int n_samples, int n_temps, int n_ladders,
                     tsu_pte3d** out) {
    TSU_ENTER(ctx);
    if (!ctx || !out) return TSU_E_INVALID;
    return pte_create(
        ctx, "pte3d", n_samples, n_temps, n_ladders, out,
        [=](tsu_pte3d* P) {
            const int rc = tsu_ising3d_create(ctx, depth, rows, cols, periodic_mask, &P->lat);
            if (rc != TSU_OK) return rc;
            P->nrows = (long long)P->lat->depth * P->lat->rows;
            P->pitch = (long long)P->lat->pitch;
            P->cols = P->lat->cols;
            P->n_axes = 3;
            P->lrows = P->lat->rows;
            P->axis_len[0] = P->lat->depth;
            P->axis_len[1] = P->lat->rows;
            P->axis_len[2] = P->lat->cols;
            P->axis_per[0] = P->lat->pz;
            P->axis_per[1] = P->lat->pr;
            P->axis_per[2] = P->lat->pc;
            P->n_dis = 4;
            return (int)TSU_OK;
        },
        pte_free);
}

int tsu_pte3d_destroy(tsu_pte3d* P) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_OK;
    (void)hipStreamSynchronize(P->ctx->stream);
    pte_free(P);
    return TSU_OK;
}

int tsu_pte3d_set_disorder(tsu_pte3d* P, const float* J_right, const float* J_down, const float* J_layer, const float* h) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const float* src[4] = {J_right, J_down, J_layer, h};
    return pte_set_disorder(
        P, src, (size_t)P->nrows * P->cols, [](tsu_pte3d* E) { return E->lat->d_dis; },
        [](tsu_ising3d* L, const float* const* a) { return tsu_ising3d_set_disorder(L, a[0], a[1], a[2], a[3]); });
}

int tsu_pte3d_set_temperatures(tsu_pte3d* P, const double* T) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_set_temperatures(P, T) : TSU_E_INVALID;
}

int tsu_pte3d_init(tsu_pte3d* P, const uint64_t* seeds, int initial) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pte_init(P, seeds, initial) : TSU_E_INVALID;
}

int tsu_pte3d_run(tsu_pte3d* P, int n_rounds, int swap_interval, int do_swap, int record) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    const int rc = pt_run_check(P, P->have_disorder, n_rounds, swap_interval);
    if (rc != TSU_OK) return rc;
    PT3Params p = pte_params(P);
    p.W = pt_group(P);
    const PTEns e = pte_ens(P, p.W);
    const dim3 og = octet_grid(make_params(P->lat));
    const dim3 grid(og.x, og.y, (unsigned)P->S * (unsigned)e.groups);
    return pt_run(
        P, n_rounds, swap_interval, do_swap, record,
        [&](uint32_t hs, int colour) {
            p.hs = hs;
            k8_pte_sweep<<<grid, 256, 0, ctx->stream>>>(p, e, colour);
        },
        pte_partials(P, p, e), [] { return (int)TSU_OK; });
}

int tsu_pte3d_history(tsu_pte3d* P, double* E, int64_t* M, int64_t* q, int32_t* walker) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_history(P, E, M, q, walker) : TSU_E_INVALID;
}

int tsu_pte3d_stats(tsu_pte3d* P, int64_t* attempts, int64_t* accepts, int64_t* round_trips, int32_t* walker_at_slot,
                    uint64_t* sweep_count, uint64_t* round_count) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_stats(P, attempts, accepts, round_trips, walker_at_slot, sweep_count, round_count) : TSU_E_INVALID;
}

int tsu_pte3d_energies(tsu_pte3d* P, double* E, int64_t* sum_s) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const PT3Params p = pte_params(P);
    const PTEns e = pte_ens(P, 1);
    return pt_energies(P, P->have_disorder, E, sum_s, pte_partials(P, p, e));
}

int tsu_pte3d_get_spins(tsu_pte3d* P, int sample, int ladder, int slot, int8_t* host) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pte_get_spins(P, sample, ladder, slot, host) : TSU_E_INVALID;
}

int tsu_pte3d_set_spins(tsu_pte3d* P, int sample, int ladder, int slot, const int8_t* host) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pte_set_spins(P, sample, ladder, slot, host) : TSU_E_INVALID;
}

int tsu_pte3d_launch_count(tsu_pte3d* P, uint64_t* n) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return pt_launch_count(P, n);
}

int tsu_pte3d_set_correlation(tsu_pte3d* P, int enable, const double* cos_z, const double* sin_z, const double* cos_r,
                              const double* sin_r, const double* cos_c, const double* sin_c) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const double* cs[3] = {cos_z, cos_r, cos_c};
    const double* sn[3] = {sin_z, sin_r, sin_c};
    return pt_set_correlation(P, enable, cs, sn);
}

int tsu_pte3d_history_modes(tsu_pte3d* P, double* modes) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_history_modes(P, modes) : TSU_E_INVALID;
}

int tsu_pte3d_set_link_overlap(tsu_pte3d* P, int enable) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_set_link_overlap(P, enable) : TSU_E_INVALID;
}

int tsu_pte3d_history_link(tsu_pte3d* P, int64_t* L) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_history_link(P, L) : TSU_E_INVALID;
}

int tsu_pte3d_profiles(tsu_pte3d* P, int sample, int slot, int64_t* p_z, int64_t* p_r, int64_t* p_c) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    int64_t* out[3] = {p_z, p_r, p_c};
    return pt_profiles(P, slot, out, sample);
}

// ------------------------------------------------------------------ population annealing
int tsu_pa3d_create(tsu_ctx* ctx, int depth, int rows, int cols, int periodic_mask, int population, tsu_pa3d** out) {
    TSU_ENTER(ctx);
    if (!ctx || !out) return TSU_E_INVALID;
    return pop_create(
        ctx, "pa3d", population, out,
        [=](tsu_pa3d* P) {
            const int rc = tsu_ising3d_create(ctx, depth, rows, cols, periodic_mask, &P->lat);
            if (rc != TSU_OK) return rc;
            P->nrows = (long long)P->lat->depth * P->lat->rows;
            P->pitch = (long long)P->lat->pitch;
            P->cols = P->lat->cols;
            P->n_axes = 3;
            P->lrows = P->lat->rows;
            P->axis_len[0] = P->lat->depth;
            P->axis_len[1] = P->lat->rows;
            P->axis_len[2] = P->lat->cols;
            P->axis_per[0] = P->lat->pz;
            P->axis_per[1] = P->lat->pr;
            P->axis_per[2] = P->lat->pc;
            return (int)TSU_OK;
        },
        pa_free);
}

int tsu_pa3d_destroy(tsu_pa3d* P) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_OK;
    (void)hipStreamSynchronize(P->ctx->stream);
    pa_free(P);
    return TSU_OK;
}

int tsu_pa3d_set_disorder(tsu_pa3d* P, const float* J_right, const float* J_down, const float* J_layer, const float* h) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    P->have_E = 0;
    return tsu_ising3d_set_disorder(P->lat, J_right, J_down, J_layer, h);
}

int tsu_pa3d_set_schedule(tsu_pa3d* P, const double* betas, int n) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pop_set_schedule(P, betas, n) : TSU_E_INVALID;
}

int tsu_pa3d_init(tsu_pa3d* P, uint64_t seed, int initial_sweeps) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    PT3Params p = pa_params(P);
    return pop_init(P, P->lat->have_disorder, seed, initial_sweeps, pa_sweep(P, p), pa_partials(P, p));
}

int tsu_pa3d_run(tsu_pa3d* P, int n_steps, int sweeps_per_step, int resample, int record) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const int rc = pop_run_check(P, P->lat->have_disorder, n_steps, sweeps_per_step);
    if (rc != TSU_OK) return rc;
    PT3Params p = pa_params(P);
    return pop_run(P, n_steps, sweeps_per_step, resample, record, pa_sweep(P, p), pa_partials(P, p));
}

int tsu_pa3d_history(tsu_pa3d* P, double* E, int64_t* M, uint32_t* W, int32_t* parent, uint64_t* S, uint64_t* U, double* E_min) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pop_history(P, E, M, W, parent, S, U, E_min) : TSU_E_INVALID;
}

int tsu_pa3d_energies(tsu_pa3d* P, double* E, int64_t* sum_s) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const PT3Params p = pa_params(P);
    return pop_energies(P, P->lat->have_disorder, E, sum_s, pa_partials(P, p));
}

int tsu_pa3d_get_spins(tsu_pa3d* P, int i, int8_t* host) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pop_get_spins(P, i, host) : TSU_E_INVALID;
}

int tsu_pa3d_set_spins(tsu_pa3d* P, int i, const int8_t* host) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pop_set_spins(P, i, host) : TSU_E_INVALID;
}

int tsu_pa3d_launch_count(tsu_pa3d* P, uint64_t* n) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return pop_launch_count(P, n);
}

int tsu_pa3d_set_overlap(tsu_pa3d* P, int enable, const double* cos_z, const double* sin_z, const double* cos_r, const double* sin_r,
                         const double* cos_c, const double* sin_c) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const double* cs[3] = {cos_z, cos_r, cos_c};
    const double* sn[3] = {sin_z, sin_r, sin_c};
    return pop_set_overlap(P, enable, cs, sn);
}

int tsu_pa3d_history_overlap(tsu_pa3d* P, int64_t* q, int64_t* L, double* modes) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pop_history_overlap(P, q, L, modes) : TSU_E_INVALID;
}

}  // extern "C"

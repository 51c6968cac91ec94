// multispin_dev.h -- what K9's kernels (multispin.hip) share on the device: the update of one site of 64 samples held in one
// 64-bit word, and the bit-sliced vertical counters of the measurement.
//
// A word holds one site of 64 disorder samples (bit set = spin +1; coupling bit set = J = -1).  For the six neighbours,
// x = neighbour word ^ coupling word has a set bit where the bond contributes +1 to the local field; a neighbour missing on an open
// axis contributes nothing.  With n present neighbours and k set bits among them the field is f = 2 k - n, an integer in -6 .. 6,
// and the contract's decision is: +1 iff u < thr(f), thr = the slot's 13-entry table (tsu_msc_thresholds).
// thr is non-decreasing in f, so for the site's one uniform u the decision of all 64 samples is "k >= k*", k* = the number of
// k in 0 .. n with u >= thr(2 k - n).  k comes from a bit-sliced adder (three count planes), and k >= k* is the carry out of
// count + (8 - k*) in three bits.  No exp, no float.
#pragma once
#include "tsu_common.h"

namespace {

struct MscGeo {
    int depth, rows, cols;
    int pz, pr, pc;   // periodic flag per axis
    int noct;         // octets per row: ceil(cols / 16)
    int nblk;         // depth * rows * noct: Philox blocks of a half-sweep
    int nsites;       // depth * rows * cols: words of a plane
};

// What every kernel takes: the planes, the couplings of the W word-planes, one table per slot and one key per (slot, replica)
struct MscParams {
    MscGeo g;
    uint64_t* s;          // plane p = (t A + a) W + w at p * nsites
    const uint64_t* j;    // J_right, J_down, J_layer: array k of word-plane w at (k W + w) * nsites
    const uint64_t* tab;  // slot t: 13 thresholds at 13 t
    const uint32_t* key;  // (slot, replica) t A + a: Philox key (k0, k1) at 2 (t A + a)
    int A, W;
};

// a + b + c of three one-bit planes: sum and carry
__device__ __forceinline__ void msc_full_add(uint64_t a, uint64_t b, uint64_t c, uint64_t& sum, uint64_t& carry) {
    sum = a ^ b ^ c;
    carry = (a & b) | (c & (a ^ b));
}

__device__ __forceinline__ uint64_t msc_maj(uint64_t a, uint64_t b, uint64_t c) { return (a & b) | (c & (a ^ b)); }

// hi16 of site m (0 .. 7) of a colour of an octet from the octet's TSU_TAG_ISING_HI block, as Octet::update takes it
__device__ __forceinline__ uint32_t msc_hi16(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, int m) {
    const uint32_t lo = (m & 2) ? w1 : w0, hi = (m & 2) ? w3 : w2;
    const uint32_t w = (m & 4) ? hi : lo;
    return ((w >> (16 * (m & 1))) & 0xFFFFu) ^ 0x8000u;
}

// k* of a site with n present neighbours for the uniform u: the number of k in 0 .. n with u >= thr(2 k - n); tie reports a
// candidate threshold whose top 16 bits equal u's
__device__ __forceinline__ int msc_kstar(const uint64_t* tab, int n, uint64_t u, bool& tie) {
    int ks = 0;
    tie = false;
#pragma unroll
    for (int k = 0; k <= 6; ++k) {
        const bool valid = k <= n;
        const uint64_t t = tab[valid ? 2 * k - n + 6 : 12];
        ks += (valid && u >= t) ? 1 : 0;
        tie = tie || (valid && (t >> 16) == (u >> 16));
    }
    return ks;
}

// The new word of site (z, r, c) of the plane at s (global memory or LDS), couplings of its word-plane at jr / jd / jl, for the site's
// hi16.  The lo16 block is drawn here, by the lane that needs it, only when hi16 ties with a candidate threshold's top half.
__device__ __forceinline__ uint64_t msc_site(const uint64_t* s, const uint64_t* __restrict__ jr, const uint64_t* __restrict__ jd,
                                             const uint64_t* __restrict__ jl, const MscGeo& g, int z, int r, int c, int q, int m,
                                             uint32_t hi, const uint64_t* tab, uint32_t hs, uint32_t k0, uint32_t k1) {
    const int R = g.rows, C = g.cols;
    const int rho = z * R + r;
    const int i = rho * C + c;
    // a missing neighbour wraps to a site that exists: every load has a valid address, what it brings is masked off
    const int ib = ((z > 0 ? z - 1 : g.depth - 1) * R + r) * C + c;
    const int jf = ((z + 1 < g.depth ? z + 1 : 0) * R + r) * C + c;
    const int iu = (z * R + (r > 0 ? r - 1 : R - 1)) * C + c;
    const int id = (z * R + (r + 1 < R ? r + 1 : 0)) * C + c;
    const int il = rho * C + (c > 0 ? c - 1 : C - 1);
    const int ir = rho * C + (c + 1 < C ? c + 1 : 0);
    const bool hb = z > 0 || g.pz, hf = z + 1 < g.depth || g.pz, hu = r > 0 || g.pr, hd = r + 1 < R || g.pr;
    const bool hl = c > 0 || g.pc, hr = c + 1 < C || g.pc;
    const uint64_t xb = hb ? s[ib] ^ jl[ib] : 0ull, xf = hf ? s[jf] ^ jl[i] : 0ull;
    const uint64_t xu = hu ? s[iu] ^ jd[iu] : 0ull, xd = hd ? s[id] ^ jd[i] : 0ull;
    const uint64_t xl = hl ? s[il] ^ jr[il] : 0ull, xr = hr ? s[ir] ^ jr[i] : 0ull;
    const int n = (int)hb + (int)hf + (int)hu + (int)hd + (int)hl + (int)hr;
    // count = b0 + 2 b1 + 4 b2
    uint64_t s1, c1, s2, c2;
    msc_full_add(xb, xf, xu, s1, c1);
    msc_full_add(xd, xl, xr, s2, c2);
    const uint64_t b0 = s1 ^ s2, c3 = s1 & s2;
    const uint64_t b1 = c1 ^ c2 ^ c3, b2 = msc_maj(c1, c2, c3);
    uint64_t u = (uint64_t)hi << 16;
    bool tie;
    int ks = msc_kstar(tab, n, u, tie);
    if (tie) {
        const u32x4 l = tsu_philox((uint32_t)q, (uint32_t)rho, hs, TSU_TAG_ISING_LO, k0, k1);
        const uint32_t lw = (m & 4) ? ((m & 2) ? l.w : l.z) : ((m & 2) ? l.y : l.x);
        u |= (lw >> (16 * (m & 1))) & 0xFFFFu;
        ks = msc_kstar(tab, n, u, tie);
    }
    // count >= k*: the carry out of count + (8 - k*) in three bits (k* = 0: every sample; k* = 7 > count: none)
    const int d = 8 - ks;
    const uint64_t d0 = (d & 1) ? ~0ull : 0ull, d1 = (d & 2) ? ~0ull : 0ull, d2 = (d & 4) ? ~0ull : 0ull;
    const uint64_t carry = msc_maj(b2, d2, msc_maj(b1, d1, b0 & d0));
    return ks == 0 ? ~0ull : carry;
}

// K one-bit planes of 64 counters: add() a one-bit word up to 2^K - 1 times, value(b) reads counter b
template <int K>
struct MscCount {
    uint64_t b[K];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int k = 0; k < K; ++k) b[k] = 0;
    }
    __device__ __forceinline__ void add(uint64_t x) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint64_t t = b[k] & x;
            b[k] ^= x;
            x = t;
        }
    }
    __device__ __forceinline__ uint32_t value(int bit) const {
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) v |= (uint32_t)((b[k] >> bit) & 1ull) << k;
        return v;
    }
};

}  // namespace

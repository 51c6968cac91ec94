// potts_kern_dev.h -- what the Potts kernels of two dimensions share on the device (K10: potts2d.hip and potts3d.hip): the Philox
// keys and the hi16 / lo16 blocks of an octet, the byte of a 16-byte load, the bond policy of the Swendsen-Wang steps and the colour
// of a cluster's root.  `r` is the row of the Philox counter: the row in 2-D, the global row rho = z R + r in 3-D.  The decision
// rule itself is potts_dev.h (host and device); the site functions, which differ in their neighbours, stay with their kernels.
#pragma once
#include "potts_dev.h"
#include "sw_dev.h"

namespace {

struct PottsKeys {
    uint32_t k0, k1, tag_hi, tag_lo;
};

// The Philox blocks of an octet's colour: hi16 at once, lo16 when the first site needs it
struct PottsDraw {
    uint32_t h0, h1, h2, h3, l0, l1, l2, l3;  // plain words: the struct stays in registers
    bool have_lo;
};

__device__ __forceinline__ PottsDraw potts_draw(const PottsKeys& k, uint32_t hs, int r, int o) {
    const u32x4 h = tsu_philox((uint32_t)o, (uint32_t)r, hs, k.tag_hi, k.k0, k.k1);
    return PottsDraw{h.x, h.y, h.z, h.w, 0, 0, 0, 0, false};
}

__device__ __forceinline__ uint32_t half_of(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, int m) {
    const uint32_t w = (m >> 1) == 0 ? w0 : ((m >> 1) == 1 ? w1 : ((m >> 1) == 2 ? w2 : w3));
    return (w >> (16 * (m & 1))) & 0xFFFFu;
}

// byte i (0 .. 15) of a 16-byte load: a colour, 0 .. 7
__device__ __forceinline__ int colour_at(const uint4& v, int i) {
    const uint32_t w = i < 4 ? v.x : (i < 8 ? v.y : (i < 12 ? v.z : v.w));
    return (int)((w >> (8 * (i & 3))) & 0xFFu);
}

struct PottsBonds {  // the bond policy: two equal colours and u < thr (thr may be 2^32: 64-bit compare)
    uint64_t thr;
    int q;
    __device__ __forceinline__ static bool sat(int sa, int sb) { return sa == sb; }
    __device__ __forceinline__ bool on(int sa, int sb, uint32_t u) const { return sa == sb && (uint64_t)u < thr; }
};

// the colour of the cluster rooted at (r, c): ((uint64)W q) >> 32, W = word c & 3 of Philox(c >> 2, r, t, tag): the word whose top
// bit is K6's coin.  Uniform over the q colours to within q 2^-32
__device__ __forceinline__ int root_colour(int r, int c, int q, uint32_t t, uint32_t tag, uint32_t k0, uint32_t k1) {
    const u32x4 w = tsu_philox((uint32_t)c >> 2, (uint32_t)r, t, tag, k0, k1);
    return (int)(((uint64_t)word_of(w, c & 3) * (uint64_t)q) >> 32);
}

}  // namespace

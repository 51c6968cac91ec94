// potts_kern_dev.h -- the device side of K10, the q-state Potts lattice, written once for DIM = 2 (potts2d.hip) and DIM = 3
// (potts3d.hip); the host side is potts_host.h, the decision rule potts_dev.h (host and device).  DIM = 2 compiles every z term out,
// as in sw_dev.h: no depth, no layer neighbour, load or bond, rows stay ints, so the 2-D kernels carry nothing of the cubic lattice.
//
// A D x R x C lattice of int8 colours (D = 1 at DIM = 2), row-major, pitch = cols, no pad (no byte that is not a site can pass for
// colour 0); global row rho = z R + r, site index i = rho C + c, one periodic flag per axis.  Everything that draws a random word
// takes rho as its row, so a one-layer lattice (1, R, C) with periodic (0, p, p) takes the 2-D colours bit for bit on every route.
//
// Heat bath, half-sweep hs = 2 sweep + colour, colour = (z + r + c) & 1.  One Philox block serves the 8 same-colour sites of 16
// consecutive columns of a global row (an octet), as in K7: hi16 of site m of the octet is half m & 1 of word m >> 1 of
// Philox(c >> 4, rho, hs, TAG_ISING_HI | rep << 8) with its top bit flipped.  The rule of potts_dev.h is monotone in u, so a site
// whose colour is the same at u = hi 2^16 and at u = hi 2^16 + 65535 is decided from hi16 alone; only the others draw the lo16 block.
//   k10_small   a lattice of at most 16384 sites in one workgroup's LDS for all sweeps of a call, a barrier per half-sweep
//   k10_sweep   one launch per half-sweep through HBM, one lane per octet.  Rows of whole octets (cols % 16 == 0): the row, the rows
//               above and below and (DIM = 3) the two layers by aligned 16-byte loads that hold sites only (three or five loads and
//               one edge byte), one 16-byte store; any other width: bounds-checked byte loads
//
// Swendsen-Wang steps share K6's and K8's machinery: the union-find of uf_dev.h, the tile geometry, seam decoder and root chase of
// sw_dev.h and the whole host side of sw_host.h.  Only what differs is here: a bond is satisfied when two colours are equal (a byte
// compare instead of a sign product), the threshold is floor(-expm1(-J / T) 2^32), and the resolve pass assigns the root's colour
// ((uint64)W q) >> 32 from the word whose top bit is K6's coin.
//   k10_sw_small   at most 16384 sites, all steps of a call in one launch
//   k10_sw_local / k10_sw_merge / k10_sw_resolve   on tiles, agent-scope atomicMin on the seams
// The three kernels that run a union-find are kernel templates, not kernels around a shared function: each reads its parameters
// directly (sw_dev.h says what a body behind a function cost K6 and K8).
//
// k10_measure: n_eq over DIM axes and N_0 .. N_7 by wave ballots, one LDS atomic per wave and word, one global atomic per workgroup
// and word.
#pragma once
#include "potts_dev.h"
#include "sw_dev.h"

namespace {

constexpr int kPottsSmallSites = 16384;
constexpr int kPottsLocalThreads = 256;  // lanes of a 2-D tile's workgroup

struct PottsGeom {
    int depth, pz, pc;   // extent and wraps that only DIM = 3 reads (DIM = 2: 1, 0 and pr), ahead of the rest: in PottsSweep, rows,
    int rows, cols, pr;  // cols, pr, the keys and hs are then one run of 8 words, which a 2-D kernel fetches at once as it always has
};

// the column wrap.  The 2-D handle has one flag for both axes (pr == pc), and its kernels read one: a second flag costs k10_small
// 2 VGPRs and k10_measure and k10_sw_small 1 each
template <int DIM, class Geom>
__device__ __forceinline__ int potts_pc(const Geom& g) {
    return DIM == 2 ? g.pr : g.pc;
}

struct PottsKeys {
    uint32_t k0, k1, tag_hi, tag_lo;
};

template <int DIM>
struct PottsSweep {
    int8_t* s;
    PottsGeom g;
    PottsKeys k;
    uint32_t hs;  // k10_sweep: the half-sweep; k10_small: the first sweep of the call
    PottsTabN<2 * DIM> t;
};

// The Philox blocks of an octet's colour: hi16 at once, lo16 when the first site needs it
struct PottsDraw {
    uint32_t h0, h1, h2, h3, l0, l1, l2, l3;  // plain words: the struct stays in registers
    bool have_lo;
};

__device__ __forceinline__ PottsDraw potts_draw(const PottsKeys& k, uint32_t hs, int rho, int o) {
    const u32x4 h = tsu_philox((uint32_t)o, (uint32_t)rho, hs, k.tag_hi, k.k0, k.k1);
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

// Site m of the octet (rho, o) with the neighbour colours nb (-1: none): its new colour
template <int NB>
__device__ __forceinline__ int potts_site(const PottsTabN<NB>& t, const PottsKeys& k, uint32_t hs, int rho, int o, int m, const int (&nb)[NB],
                                          PottsDraw& d) {
    double Z[TSU_POTTS_MAX_Q];
    potts_cum(t, nb, Z);
    const uint32_t hi = half_of(d.h0, d.h1, d.h2, d.h3, m) ^ 0x8000u;
    int col = potts_pick(Z, t.q, hi << 16);
    if (col != potts_pick(Z, t.q, (hi << 16) | 0xFFFFu)) {  // the low half decides: K1's lo16 block
        if (!d.have_lo) {
            const u32x4 l = tsu_philox((uint32_t)o, (uint32_t)rho, hs, k.tag_lo, k.k0, k.k1);
            d.l0 = l.x;
            d.l1 = l.y;
            d.l2 = l.z;
            d.l3 = l.w;
            d.have_lo = true;
        }
        const uint32_t lo = half_of(d.l0, d.l1, d.l2, d.l3, m);
        col = potts_pick(Z, t.q, (hi << 16) | lo);
    }
    return col;
}

// the global rows of the neighbour rows of (z, r): above and below in the layer, DIM = 3: the same row of the layers below and
// above (-1: none)
struct PottsRows {
    int ru, rd, rzm, rzp;
};

template <int DIM>
__device__ __forceinline__ PottsRows potts_rows(const PottsGeom& g, int z, int r) {
    const int rho = (DIM == 3 ? z * g.rows : 0) + r;
    PottsRows n;
    n.ru = r > 0 ? rho - 1 : (g.pr ? rho + g.rows - 1 : -1);
    n.rd = r + 1 < g.rows ? rho + 1 : (g.pr ? rho - r : -1);
    n.rzm = n.rzp = -1;
    if constexpr (DIM == 3) {
        n.rzm = z > 0 ? rho - g.rows : (g.pz ? (g.depth - 1) * g.rows + r : -1);
        n.rzp = z + 1 < g.depth ? rho + g.rows : (g.pz ? r : -1);
    }
    return n;
}

// One colour of the octet (rho, o): sites c = 16 o + 2 m + par, m = 0 .. 7.  s: the lattice in HBM or LDS, pitch = cols.  The sites
// written have this half-sweep's colour, the sites read the other one.  Every index stays inside [0, depth rows cols)
template <int DIM>
__device__ __forceinline__ void potts_octet(int8_t* s, const PottsGeom& g, const PottsTabN<2 * DIM>& t, const PottsKeys& k, uint32_t hs,
                                            int rho, int o, int colour) {
    const int z = DIM == 3 ? rho / g.rows : 0, r = rho - z * g.rows;
    const int par = (z + r + colour) & 1, c0 = 16 * o;
    const PottsRows n = potts_rows<DIM>(g, z, r);
    const long long row = (long long)rho * g.cols;
    PottsDraw d = potts_draw(k, hs, rho, o);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int c = c0 + 2 * m + par;
        if (c >= g.cols) break;
        const int cl = c > 0 ? c - 1 : (potts_pc<DIM>(g) ? g.cols - 1 : -1);
        const int cr = c + 1 < g.cols ? c + 1 : (potts_pc<DIM>(g) ? 0 : -1);
        int nb[2 * DIM];  // DIM = 3: the layers first
        if constexpr (DIM == 3) {
            nb[0] = n.rzm >= 0 ? s[(long long)n.rzm * g.cols + c] : -1;
            nb[1] = n.rzp >= 0 ? s[(long long)n.rzp * g.cols + c] : -1;
        }
        nb[2 * DIM - 4] = n.ru >= 0 ? s[(long long)n.ru * g.cols + c] : -1;
        nb[2 * DIM - 3] = n.rd >= 0 ? s[(long long)n.rd * g.cols + c] : -1;
        nb[2 * DIM - 2] = cl >= 0 ? s[row + cl] : -1;
        nb[2 * DIM - 1] = cr >= 0 ? s[row + cr] : -1;
        s[row + c] = (int8_t)potts_site(t, k, hs, rho, o, m, nb, d);
    }
}

// The same half-sweep of an octet of a lattice whose rows are whole octets (cols % 16 == 0, so every 16-byte row segment is aligned
// and holds sites only): three (DIM = 3: five) 16-byte loads and one edge byte instead of byte loads, one 16-byte store (the other
// colour's bytes go back as read; nobody writes them in this launch).  PAR = the parity of the colour's columns in this row
template <int DIM, int PAR>
__device__ __forceinline__ void potts_octet_rows16(int8_t* s, const PottsGeom& g, const PottsTabN<2 * DIM>& t, const PottsKeys& k,
                                                   uint32_t hs, int z, int r, int o) {
    const int c0 = 16 * o, rho = (DIM == 3 ? z * g.rows : 0) + r;
    const PottsRows n = potts_rows<DIM>(g, z, r);
    const long long row = (long long)rho * g.cols;
    const uint4 C = *reinterpret_cast<const uint4*>(s + row + c0);
    // a missing row or layer is loaded from this row (a valid address, no branch); what it brings is never used
    const uint4 U = *reinterpret_cast<const uint4*>(s + (long long)(n.ru >= 0 ? n.ru : rho) * g.cols + c0);
    const uint4 D = *reinterpret_cast<const uint4*>(s + (long long)(n.rd >= 0 ? n.rd : rho) * g.cols + c0);
    uint4 A = {}, B = {};
    if constexpr (DIM == 3) {
        A = *reinterpret_cast<const uint4*>(s + (long long)(n.rzm >= 0 ? n.rzm : rho) * g.cols + c0);
        B = *reinterpret_cast<const uint4*>(s + (long long)(n.rzp >= 0 ? n.rzp : rho) * g.cols + c0);
    }
    // the one neighbour outside the 16 bytes: left of position 0 (PAR = 0) or right of position 15 (PAR = 1)
    const int pc = potts_pc<DIM>(g);
    const int ce = PAR == 0 ? (c0 > 0 ? c0 - 1 : (pc ? g.cols - 1 : -1)) : (c0 + 16 < g.cols ? c0 + 16 : (pc ? 0 : -1));
    const int s_edge = ce >= 0 ? (int)s[row + ce] : -1;
    PottsDraw d = potts_draw(k, hs, rho, o);
    uint32_t o0 = C.x, o1 = C.y, o2 = C.z, o3 = C.w;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int i = 2 * m + PAR;
        int nb[2 * DIM];
        if constexpr (DIM == 3) {
            nb[0] = n.rzm >= 0 ? colour_at(A, i) : -1;
            nb[1] = n.rzp >= 0 ? colour_at(B, i) : -1;
        }
        nb[2 * DIM - 4] = n.ru >= 0 ? colour_at(U, i) : -1;
        nb[2 * DIM - 3] = n.rd >= 0 ? colour_at(D, i) : -1;
        nb[2 * DIM - 2] = i > 0 ? colour_at(C, i - 1) : s_edge;
        nb[2 * DIM - 1] = i < 15 ? colour_at(C, i + 1) : s_edge;
        const uint32_t col = (uint32_t)potts_site(t, k, hs, rho, o, m, nb, d);
        const int sh = 8 * (i & 3);
        uint32_t& w = (i >> 2) == 0 ? o0 : ((i >> 2) == 1 ? o1 : ((i >> 2) == 2 ? o2 : o3));
        w = (w & ~(0xFFu << sh)) | (col << sh);
    }
    *reinterpret_cast<uint4*>(s + row + c0) = make_uint4(o0, o1, o2, o3);
}

// ROWS16: the lattice's rows are whole octets (the host's choice; two instantiations, so that neither carries the other's registers)
template <int DIM, bool ROWS16>
__global__ __launch_bounds__(256) void k10_sweep(PottsSweep<DIM> p) {
    const int noct = (p.g.cols + 15) >> 4;
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= (long long)(DIM == 3 ? p.g.depth : 1) * p.g.rows * noct) return;
    const int rho = (int)(lane / noct), o = (int)(lane - (long long)rho * noct);
    const int colour = (int)(p.hs & 1u);
    if constexpr (!ROWS16) {
        potts_octet<DIM>(p.s, p.g, p.t, p.k, p.hs, rho, o, colour);
    } else {
        const int z = DIM == 3 ? rho / p.g.rows : 0, r = rho - z * p.g.rows;
        if (((z + r + colour) & 1) == 0) potts_octet_rows16<DIM, 0>(p.s, p.g, p.t, p.k, p.hs, z, r, o);
        else potts_octet_rows16<DIM, 1>(p.s, p.g, p.t, p.k, p.hs, z, r, o);
    }
}

template <int DIM>
__global__ __launch_bounds__(kSwMaxThreads) void k10_small(PottsSweep<DIM> p, int n_sweeps) {
    __shared__ int8_t s_sp[kPottsSmallSites];
    const int nrows = (DIM == 3 ? p.g.depth : 1) * p.g.rows, n = nrows * p.g.cols;  // n <= kPottsSmallSites: the host's route
    const int tid = threadIdx.x, nt = blockDim.x;
    const int noct = (p.g.cols + 15) >> 4, nlanes = nrows * noct;
    for (int i = tid; i < n; i += nt) s_sp[i] = p.s[i];
    __syncthreads();
    for (int s = 0; s < n_sweeps; ++s) {
#pragma unroll 1
        for (int colour = 0; colour < 2; ++colour) {
            const uint32_t hs = 2u * (p.hs + (uint32_t)s) + (uint32_t)colour;
            for (int l = tid; l < nlanes; l += nt) {
                const int rho = l / noct, o = l - rho * noct;
                potts_octet<DIM>(s_sp, p.g, p.t, p.k, hs, rho, o, colour);
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < n; i += nt) p.s[i] = s_sp[i];
}

// ---------------------------------------------------------------- observables
struct PottsMeasure {
    const int8_t* s;
    PottsGeom g;
    int q;
    unsigned long long* row;  // 9 words, zeroed on the stream ahead of the launch
};

template <int DIM>
__global__ __launch_bounds__(256) void k10_measure(PottsMeasure p) {
    __shared__ unsigned long long s_row[TSU_POTTS_RECORD_WORDS];
    if (threadIdx.x < TSU_POTTS_RECORD_WORDS) s_row[threadIdx.x] = 0;
    __syncthreads();
    const long long plane = (long long)p.g.rows * p.g.cols, n = plane * (DIM == 3 ? p.g.depth : 1);
    unsigned long long acc[TSU_POTTS_RECORD_WORDS] = {};  // wave-uniform: every lane of a wave holds the wave's counts
    for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {  // whole waves stay in
        const long long i = base + threadIdx.x;
        const bool valid = i < n;
        int col = -1;
        bool eq_r = false, eq_d = false, eq_l = false;
        if (valid) {
            const int z = DIM == 3 ? (int)(i / plane) : 0;
            const long long rem = i - (long long)z * plane;
            const int r = (int)(rem / p.g.cols), c = (int)(rem - (long long)r * p.g.cols);
            col = p.s[i];
            const int cr = c + 1 < p.g.cols ? c + 1 : (potts_pc<DIM>(p.g) ? 0 : -1);
            const int rd = r + 1 < p.g.rows ? r + 1 : (p.g.pr ? 0 : -1);
            eq_r = cr >= 0 && p.s[(long long)z * plane + (long long)r * p.g.cols + cr] == col;
            eq_d = rd >= 0 && p.s[(long long)z * plane + (long long)rd * p.g.cols + c] == col;
            if constexpr (DIM == 3) {
                const int zl = z + 1 < p.g.depth ? z + 1 : (p.g.pz ? 0 : -1);
                eq_l = zl >= 0 && p.s[(long long)zl * plane + rem] == col;
            }
        }
        int n_eq = __popcll(__ballot(eq_r)) + __popcll(__ballot(eq_d));
        if constexpr (DIM == 3) n_eq += __popcll(__ballot(eq_l));
        acc[0] += (unsigned long long)n_eq;
#pragma unroll
        for (int c = 0; c < TSU_POTTS_MAX_Q; ++c)
            if (c < p.q) acc[1 + c] += (unsigned long long)__popcll(__ballot(col == c));
    }
    if ((threadIdx.x & 63u) == 0) {
#pragma unroll
        for (int k = 0; k < TSU_POTTS_RECORD_WORDS; ++k)
            if (acc[k] != 0) atomicAdd(&s_row[k], acc[k]);
    }
    __syncthreads();
    if (threadIdx.x < TSU_POTTS_RECORD_WORDS && s_row[threadIdx.x] != 0) atomicAdd(&p.row[threadIdx.x], s_row[threadIdx.x]);
}

// ---------------------------------------------------------------- Swendsen-Wang steps
struct PottsBonds {  // the bond policy: two equal colours and u < thr (thr may be 2^32: 64-bit compare)
    uint64_t thr;
    int q;
    __device__ __forceinline__ static bool sat(int sa, int sb) { return sa == sb; }
    __device__ __forceinline__ bool on(int sa, int sb, uint32_t u) const { return sa == sb && (uint64_t)u < thr; }
};

using PottsItem = SwItem<PottsBonds>;
using PottsParams = SwParams<PottsBonds>;

// the colour of the cluster rooted at (rho, c): ((uint64)W q) >> 32, W = word c & 3 of Philox(c >> 2, rho, t, tag): the word whose
// top bit is K6's coin.  Uniform over the q colours to within q 2^-32
__device__ __forceinline__ int root_colour(int rho, int c, int q, uint32_t t, uint32_t tag, uint32_t k0, uint32_t k1) {
    const u32x4 w = tsu_philox((uint32_t)c >> 2, (uint32_t)rho, t, tag, k0, k1);
    return (int)(((uint64_t)word_of(w, c & 3) * (uint64_t)q) >> 32);
}

// Rec: always empty (the Potts handle keeps no cluster-size records); the pack is there because sw_host.h names a measured
// instantiation of every one-workgroup kernel.  LDS: 4 B labels + 1 B colours a site (the host's dynamic size), n <= 16384
template <int DIM, class... Rec>
__global__ __launch_bounds__(kSwMaxThreads) void k10_sw_small(const PottsItem* __restrict__ items, PottsItem one, SwGeom g, int n_steps, int* err,
                                                              Rec...) {
    extern __shared__ int s_lab[];
    __shared__ int s_bad;
    const PottsItem& it = items ? items[blockIdx.x] : one;
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    const int rows = g.rows, cols = g.cols, pr = g.pr, pc = potts_pc<DIM>(g);
    const int nrows = (DIM == 3 ? g.depth : 1) * rows, n = nrows * cols, tid = threadIdx.x, nt = blockDim.x;
    int8_t* const s_spin = reinterpret_cast<int8_t*>(s_lab + n);
    if (tid == 0) s_bad = 0;
    for (int i = tid; i < n; i += nt) s_spin[i] = it.s[i];
    const int hc = (cols + 1) >> 1, npairs = nrows * hc;
    for (int s = 0; s < n_steps; ++s) {
        const uint32_t t = it.k.t + (uint32_t)s;
        for (int i = tid; i < n; i += nt) s_lab[i] = i;
        __syncthreads();
        int budget = kBudget;
        for (int p = tid; p < npairs; p += nt) {
            const int rho = p / hc, cp = p - rho * hc;
            const int z = DIM == 3 ? rho / rows : 0, r = rho - z * rows;
            const u32x4 w = tsu_philox((uint32_t)cp, (uint32_t)rho, t, it.k.tag_bond, it.k.k0, it.k.k1);
            const int rd = r + 1 < rows ? rho + 1 : (pr ? z * rows : -1);  // global row of the down neighbour
            // DIM = 3: the global row of the layer neighbour, and the layer bonds' block, drawn once a site of the pair has a layer
            // neighbour of its colour
            [[maybe_unused]] int rf = -1;
            if constexpr (DIM == 3) rf = z + 1 < g.depth ? rho + rows : (g.pz ? r : -1);
            [[maybe_unused]] u32x4 wl = {0u, 0u, 0u, 0u};
            [[maybe_unused]] bool have_wl = false;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = 2 * cp + j;
                if (c >= cols) break;
                const int i = rho * cols + c, si = s_spin[i];
                const int cr = c + 1 < cols ? c + 1 : (pc ? 0 : -1);
                if (cr >= 0 && it.b.on(si, s_spin[rho * cols + cr], j ? w.z : w.x))
                    if (!uf_union<false, WG>(s_lab, i, rho * cols + cr, budget)) s_bad = 1;
                if (rd >= 0 && it.b.on(si, s_spin[rd * cols + c], j ? w.w : w.y))
                    if (!uf_union<false, WG>(s_lab, i, rd * cols + c, budget)) s_bad = 1;
                if constexpr (DIM == 3) {
                    if (rf >= 0 && PottsBonds::sat(si, s_spin[rf * cols + c])) {
                        if (!have_wl) wl = tsu_philox((uint32_t)cp >> 1, (uint32_t)rho, t, it.k.tag_layer, it.k.k0, it.k.k1);
                        have_wl = true;
                        if ((uint64_t)word_of(wl, c & 3) < it.b.thr)
                            if (!uf_union<false, WG>(s_lab, i, rf * cols + c, budget)) s_bad = 1;
                    }
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < n; i += nt) {
            budget = kBudget;
            const int root = uf_find<false, WG>(s_lab, i, budget);
            if (budget < 0) s_bad = 1;
            const int rr = root / cols, rc = root - rr * cols;
            s_spin[i] = (int8_t)root_colour(rr, rc, it.b.q, t, it.k.tag_flip, it.k.k0, it.k.k1);
        }
        __syncthreads();
        if (s_bad) break;
    }
    if (s_bad) {
        if (tid == 0) raise_err(err);
        return;  // the lattice keeps its colours from before the call
    }
    for (int i = tid; i < n; i += nt) it.s[i] = s_spin[i];
}

// tile blockIdx.x (row-major over nz x nr x nc) of tz x tr x tc sites (DIM = 2: tz = nz = 1); bonds with both ends in the tile, none
// across its faces or a wrap.  LDS: tz*tr*tc int32 labels (tile-local, row-major: the same order as the global indices inside a
// tile) and as many colours.  Writes the global index of every site's tile root.  DIM = 2: 256 lanes a tile, a constant stride and
// int rows; DIM = 3: the host's lane count (up to 1024) and long long global rows
template <int DIM>
__global__ __launch_bounds__(DIM == 2 ? kPottsLocalThreads : kSwMaxThreads) void k10_sw_local(PottsParams p) {
    extern __shared__ int s_lab[];
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    const int TZ = DIM == 3 ? p.g.tz : 1, TR = p.g.tr, TC = p.g.tc, n = TZ * TR * TC;
    int8_t* const s_spin = reinterpret_cast<int8_t*>(s_lab + n);
    const int bz = DIM == 3 ? (int)(blockIdx.x / (unsigned)(p.g.nr * p.g.nc)) : 0, brc = (int)blockIdx.x - bz * p.g.nr * p.g.nc;
    // the tile's row: an unsigned division at DIM = 2, a signed one at DIM = 3, as each local pass has always been compiled
    const int br = DIM == 2 ? (int)((unsigned)brc / (unsigned)p.g.nc) : brc / p.g.nc, bc = brc - br * p.g.nc;
    const int z0 = bz * TZ, r0 = br * TR, c0 = bc * TC;
    const int tz = DIM == 3 ? (p.g.depth - z0 < TZ ? p.g.depth - z0 : TZ) : 1;
    const int tr = p.g.rows - r0 < TR ? p.g.rows - r0 : TR, tc = p.g.cols - c0 < TC ? p.g.cols - c0 : TC;
    const int tid = threadIdx.x, nt = DIM == 2 ? kPottsLocalThreads : (int)blockDim.x;
    for (int i = tid; i < n; i += nt) {
        const int lz = DIM == 3 ? i / (TR * TC) : 0, rem = i - lz * TR * TC, lr = rem / TC, lc = rem - lr * TC;
        const sw_row_t<DIM> rho = (sw_row_t<DIM>)(z0 + lz) * p.g.rows + r0 + lr;
        s_lab[i] = i;
        s_spin[i] = (lz < tz && lr < tr && lc < tc) ? p.s[(long long)rho * p.g.pitch + c0 + lc] : (int8_t)-1;  // outside: no colour
    }
    __syncthreads();
    int budget = kBudget;
    bool bad = false;
    const int hw = TC >> 1;
    for (int q = tid; q < TZ * TR * hw; q += nt) {
        const int lz = DIM == 3 ? q / (TR * hw) : 0, rem = q - lz * TR * hw, lr = rem / hw, lc0 = 2 * (rem - lr * hw);
        if (lz >= tz || lr >= tr || lc0 >= tc) continue;
        const sw_row_t<DIM> rho = (sw_row_t<DIM>)(z0 + lz) * p.g.rows + r0 + lr;
        const u32x4 w = tsu_philox((uint32_t)(c0 + lc0) >> 1, (uint32_t)rho, p.k.t, p.k.tag_bond, p.k.k0, p.k.k1);
        [[maybe_unused]] u32x4 wl = {0u, 0u, 0u, 0u};
        [[maybe_unused]] bool have_wl = false;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int lc = lc0 + j;
            if (lc >= tc) break;
            const int i = (lz * TR + lr) * TC + lc, si = s_spin[i];
            if (lc + 1 < tc && p.b.on(si, s_spin[i + 1], j ? w.z : w.x)) bad |= !uf_union<false, WG>(s_lab, i, i + 1, budget);
            if (lr + 1 < tr && p.b.on(si, s_spin[i + TC], j ? w.w : w.y)) bad |= !uf_union<false, WG>(s_lab, i, i + TC, budget);
            if constexpr (DIM == 3) {
                if (lz + 1 < tz && PottsBonds::sat(si, s_spin[i + TR * TC])) {
                    if (!have_wl) wl = tsu_philox((uint32_t)(c0 + lc0) >> 2, (uint32_t)rho, p.k.t, p.k.tag_layer, p.k.k0, p.k.k1);
                    have_wl = true;
                    if ((uint64_t)word_of(wl, (c0 + lc) & 3) < p.b.thr) bad |= !uf_union<false, WG>(s_lab, i, i + TR * TC, budget);
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += nt) {
        const int lz = DIM == 3 ? i / (TR * TC) : 0, rem = i - lz * TR * TC, lr = rem / TC, lc = rem - lr * TC;
        if (lz >= tz || lr >= tr || lc >= tc) continue;
        budget = kBudget;
        const int root = uf_find<false, WG>(s_lab, i, budget);
        bad |= budget < 0;
        const int rz = DIM == 3 ? root / (TR * TC) : 0, rrem = root - rz * TR * TC, rr = rrem / TC, rc = rrem - rr * TC;
        const sw_row_t<DIM> rho = (sw_row_t<DIM>)(z0 + lz) * p.g.rows + r0 + lr;
        p.labels[(long long)rho * p.g.cols + c0 + lc] = ((z0 + rz) * p.g.rows + r0 + rr) * p.g.cols + c0 + rc;
    }
    if (bad) raise_err(p.err);
}

// one lane per bond across a tile face or a wrap (sw_seam: column seams, row seams, DIM = 3: layer seams)
template <int DIM>
__global__ __launch_bounds__(256) void k10_sw_merge(PottsParams p) {
    sw_row_t<DIM> rho, rho2;
    int c, c2;
    const int axis = sw_seam<DIM>(p.g, (long long)blockIdx.x * 256 + threadIdx.x, rho, c, rho2, c2);
    if (axis < 0) return;
    const int sa = p.s[(long long)rho * p.g.pitch + c], sb = p.s[(long long)rho2 * p.g.pitch + c2];
    if (!PottsBonds::sat(sa, sb)) return;
    uint32_t u;
    if (DIM == 3 && axis == 2) {
        u = word_of(tsu_philox((uint32_t)c >> 2, (uint32_t)rho, p.k.t, p.k.tag_layer, p.k.k0, p.k.k1), c & 3);
    } else {
        const u32x4 w = tsu_philox((uint32_t)c >> 1, (uint32_t)rho, p.k.t, p.k.tag_bond, p.k.k0, p.k.k1);
        // word 2 (c & 1) + axis, spelt per dimension as each merge pass has always been compiled (word_of costs DIM = 2 two VGPRs)
        if constexpr (DIM == 2) u = axis ? ((c & 1) ? w.w : w.y) : ((c & 1) ? w.z : w.x);
        else u = word_of(w, 2 * (c & 1) + axis);
    }
    if ((uint64_t)u >= p.b.thr) return;
    int budget = kBudget;
    const int a = p.labels[(long long)rho * p.g.cols + c], b = p.labels[(long long)rho2 * p.g.cols + c2];
    if (!uf_union<false, __HIP_MEMORY_SCOPE_AGENT>(p.labels, a, b, budget)) raise_err(p.err);
}

// one lane per 4 sites of a global row: the root of each site (labels only: no lane reads a colour another lane writes, and no
// union-find runs), the root's colour (one Philox block per distinct root of the lane), the colour stored as a byte
template <int DIM>
__global__ __launch_bounds__(256) void k10_sw_resolve(PottsParams p, int quads) {
    const SwGeom& g = p.g;
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    const sw_row_t<DIM> rho = (sw_row_t<DIM>)(lane / quads);
    const int c0 = 4 * (int)(lane - (long long)rho * quads);
    if (rho >= (sw_row_t<DIM>)(DIM == 3 ? g.depth : 1) * g.rows) return;
    int last = -1, last_colour = 0;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (c0 + j >= g.cols) break;
        const int x = sw_chase<false>(p.labels, p.labels[(long long)rho * g.cols + c0 + j], bad);
        if (x != last) {
            const int rr = x / g.cols, rc = x - rr * g.cols;
            last = x;
            last_colour = root_colour(rr, rc, p.b.q, p.k.t, p.k.tag_flip, p.k.k0, p.k.k1);
        }
        p.s[(long long)rho * g.pitch + c0 + j] = (int8_t)last_colour;
    }
    if (bad) raise_err(p.err);
}

}  // namespace

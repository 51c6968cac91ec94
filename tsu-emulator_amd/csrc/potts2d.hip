// potts2d.hip -- K10: q-state Potts lattices in 2-D on a handle of their own (gfx950): heat-bath sweeps, Swendsen-Wang steps and
// exact integer observables (include/tsu_hip_potts.h; the contracts are DESIGN.md section 3).
//
// Heat bath, half-sweep hs = 2 sweep + colour, colour = (r + c) & 1.  One Philox block serves the 8 same-colour sites of 16
// consecutive columns of a row (an octet), as in K7: hi16 of site m of the octet is half m & 1 of word m >> 1 of
// Philox(c >> 4, r, hs, TAG_ISING_HI | rep << 8) with its top bit flipped.  The rule of potts_dev.h is monotone in u, so a site whose
// colour is the same at u = hi 2^16 and at u = hi 2^16 + 65535 is decided from hi16 alone; only the others draw the lo16 block.
//   k10_small   a lattice of at most 16384 sites in one workgroup's LDS for all sweeps of a call, a barrier per half-sweep
//   k10_sweep   one launch per half-sweep through HBM, one lane per octet (two instantiations: rows of whole octets, any width)
// The state has no pad: the pitch is cols, so no byte that is not a site can pass for colour 0.  Neighbours are read by
// bounds-checked byte loads, or, where the rows are whole octets (cols % 16 == 0), by aligned 16-byte loads that hold sites only.
//
// Swendsen-Wang steps share K6's machinery: the union-find of uf_dev.h, the seam decoder and root chase of sw_dev.h and the whole
// host side of sw_host.h through the traits struct K10 below.  Only what differs is here: a bond is satisfied when two colours are
// equal (a byte compare instead of a sign product), the threshold is floor(-expm1(-J / T) 2^32), and the resolve pass assigns the
// root's colour ((uint64)W q) >> 32 from the word whose top bit is K6's coin.
//   k10_sw_small   at most 16384 sites, all steps of a call in one launch
//   k10_sw_local / k10_sw_merge / k10_sw_resolve   on tiles, agent-scope atomicMin on the seams
//
// k10_measure: n_eq and N_0 .. N_7 by wave ballots, one LDS atomic per wave and word, one global atomic per workgroup and word.
#include <math.h>
#include <stdlib.h>

#include <vector>

#include "potts_dev.h"
#include "potts_kern_dev.h"
#include "sw_host.h"

struct tsu_potts2d {
    tsu_ctx* ctx;
    int rows, cols, q, periodic;
    int8_t* d_s;  // rows * cols colours, pitch = cols
    double J;
    double h[TSU_POTTS_MAX_Q];
    int* h_err;         // host-mapped flag of the cluster kernels (2: a capped union / find loop expired)
    tsu_sw_scratch sw;  // labels and launches of the cluster steps
    long long* d_obs;   // one measurement row
    long long* d_rec;   // the rows of the most recent run
    size_t rec_cap;
    int rec_rows;
    unsigned long long launches;  // heat-bath and measuring launches
};

namespace {

constexpr int kTile = 64;
constexpr int kLocalThreads = 256;
constexpr int kSmallSites = 16384;

struct PottsGeom {
    int rows, cols, periodic;
};

struct PottsSweep {
    int8_t* s;
    PottsGeom g;
    PottsKeys k;
    uint32_t hs;  // k10_sweep: the half-sweep; k10_small: the first sweep of the call
    PottsTab t;
};

// Site m of the octet (r, o) with the neighbour colours up, dn, lf, rt (-1: none): its new colour
__device__ __forceinline__ int potts_site(const PottsTab& t, const PottsKeys& k, uint32_t hs, int r, int o, int m, int up, int dn, int lf,
                                          int rt, PottsDraw& d) {
    double Z[TSU_POTTS_MAX_Q];
    potts_cum(t, up, dn, lf, rt, Z);
    const uint32_t hi = half_of(d.h0, d.h1, d.h2, d.h3, m) ^ 0x8000u;
    int col = potts_pick(Z, t.q, hi << 16);
    if (col != potts_pick(Z, t.q, (hi << 16) | 0xFFFFu)) {  // the low half decides: K1's lo16 block
        if (!d.have_lo) {
            const u32x4 l = tsu_philox((uint32_t)o, (uint32_t)r, hs, k.tag_lo, k.k0, k.k1);
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

// One colour of the octet (r, o): sites c = 16 o + 2 m + par, m = 0 .. 7.  S gives at(r, c) and put(r, c, v) on HBM or LDS.  The sites
// written have this half-sweep's colour, the sites read the other one
template <class S>
__device__ __forceinline__ void potts_octet(S sp, const PottsGeom& g, const PottsTab& t, const PottsKeys& k, uint32_t hs, int r, int o,
                                            int colour) {
    const int par = (r + colour) & 1, c0 = 16 * o;
    const int ru = r > 0 ? r - 1 : (g.periodic ? g.rows - 1 : -1);
    const int rd = r + 1 < g.rows ? r + 1 : (g.periodic ? 0 : -1);
    PottsDraw d = potts_draw(k, hs, r, o);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int c = c0 + 2 * m + par;
        if (c >= g.cols) break;
        const int cl = c > 0 ? c - 1 : (g.periodic ? g.cols - 1 : -1);
        const int cr = c + 1 < g.cols ? c + 1 : (g.periodic ? 0 : -1);
        const int up = ru >= 0 ? sp.at(ru, c) : -1, dn = rd >= 0 ? sp.at(rd, c) : -1;
        const int lf = cl >= 0 ? sp.at(r, cl) : -1, rt = cr >= 0 ? sp.at(r, cr) : -1;
        sp.put(r, c, potts_site(t, k, hs, r, o, m, up, dn, lf, rt, d));
    }
}

struct PottsPlane {  // a lattice in HBM or LDS, pitch = cols
    int8_t* s;
    int cols;
    __device__ __forceinline__ int at(int r, int c) const { return s[(long long)r * cols + c]; }
    __device__ __forceinline__ void put(int r, int c, int v) const { s[(long long)r * cols + c] = (int8_t)v; }
};

// The same half-sweep of an octet of a lattice whose rows are whole octets (cols % 16 == 0, so every 16-byte row segment is aligned
// and holds sites only): three 16-byte loads and one edge byte instead of 32 byte loads, one 16-byte store (the other colour's bytes
// go back as read; nobody writes them in this launch).  PAR = the parity of the colour's columns in this row
template <int PAR>
__device__ __forceinline__ void potts_octet_rows16(int8_t* s, const PottsGeom& g, const PottsTab& t, const PottsKeys& k, uint32_t hs, int r,
                                                   int o) {
    const int c0 = 16 * o;
    const int ru = r > 0 ? r - 1 : (g.periodic ? g.rows - 1 : -1);
    const int rd = r + 1 < g.rows ? r + 1 : (g.periodic ? 0 : -1);
    const long long row = (long long)r * g.cols;
    const uint4 C = *reinterpret_cast<const uint4*>(s + row + c0);
    // a missing row is loaded from this row (a valid address, no branch); what it brings is never used
    const uint4 U = *reinterpret_cast<const uint4*>(s + (long long)(ru >= 0 ? ru : r) * g.cols + c0);
    const uint4 D = *reinterpret_cast<const uint4*>(s + (long long)(rd >= 0 ? rd : r) * g.cols + c0);
    // the one neighbour outside the 16 bytes: left of position 0 (PAR = 0) or right of position 15 (PAR = 1)
    const int ce = PAR == 0 ? (c0 > 0 ? c0 - 1 : (g.periodic ? g.cols - 1 : -1)) : (c0 + 16 < g.cols ? c0 + 16 : (g.periodic ? 0 : -1));
    const int s_edge = ce >= 0 ? (int)s[row + ce] : -1;
    PottsDraw d = potts_draw(k, hs, r, o);
    uint32_t o0 = C.x, o1 = C.y, o2 = C.z, o3 = C.w;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int i = 2 * m + PAR;
        const int up = ru >= 0 ? colour_at(U, i) : -1, dn = rd >= 0 ? colour_at(D, i) : -1;
        const int lf = i > 0 ? colour_at(C, i - 1) : s_edge, rt = i < 15 ? colour_at(C, i + 1) : s_edge;
        const uint32_t col = (uint32_t)potts_site(t, k, hs, r, o, m, up, dn, lf, rt, d);
        const int sh = 8 * (i & 3);
        uint32_t& w = (i >> 2) == 0 ? o0 : ((i >> 2) == 1 ? o1 : ((i >> 2) == 2 ? o2 : o3));
        w = (w & ~(0xFFu << sh)) | (col << sh);
    }
    *reinterpret_cast<uint4*>(s + row + c0) = make_uint4(o0, o1, o2, o3);
}

// ROWS16: the lattice's rows are whole octets (the host's choice; two instantiations, so that neither carries the other's registers)
template <bool ROWS16>
__global__ __launch_bounds__(256) void k10_sweep(PottsSweep p) {
    const int noct = (p.g.cols + 15) >> 4;
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= (long long)p.g.rows * noct) return;
    const int r = (int)(lane / noct), o = (int)(lane - (long long)r * noct);
    const int colour = (int)(p.hs & 1u);
    if constexpr (!ROWS16) {
        potts_octet(PottsPlane{p.s, p.g.cols}, p.g, p.t, p.k, p.hs, r, o, colour);
    } else {
        if (((r + colour) & 1) == 0) potts_octet_rows16<0>(p.s, p.g, p.t, p.k, p.hs, r, o);
        else potts_octet_rows16<1>(p.s, p.g, p.t, p.k, p.hs, r, o);
    }
}

__global__ __launch_bounds__(kSwMaxThreads) void k10_small(PottsSweep p, int n_sweeps) {
    __shared__ int8_t s_sp[kSmallSites];
    const int n = p.g.rows * p.g.cols, tid = threadIdx.x, nt = blockDim.x;
    const int noct = (p.g.cols + 15) >> 4, nlanes = p.g.rows * noct;
    for (int i = tid; i < n; i += nt) s_sp[i] = p.s[i];
    __syncthreads();
    for (int s = 0; s < n_sweeps; ++s) {
#pragma unroll 1
        for (int colour = 0; colour < 2; ++colour) {
            const uint32_t hs = 2u * (p.hs + (uint32_t)s) + (uint32_t)colour;
            for (int l = tid; l < nlanes; l += nt) {
                const int r = l / noct, o = l - r * noct;
                potts_octet(PottsPlane{s_sp, p.g.cols}, p.g, p.t, p.k, hs, r, o, colour);
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

__global__ __launch_bounds__(256) void k10_measure(PottsMeasure p) {
    __shared__ unsigned long long s_row[TSU_POTTS_RECORD_WORDS];
    if (threadIdx.x < TSU_POTTS_RECORD_WORDS) s_row[threadIdx.x] = 0;
    __syncthreads();
    const long long n = (long long)p.g.rows * p.g.cols;
    unsigned long long acc[TSU_POTTS_RECORD_WORDS] = {};  // wave-uniform: every lane of a wave holds the wave's counts
    for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {  // whole waves stay in
        const long long i = base + threadIdx.x;
        const bool valid = i < n;
        int col = -1;
        bool eq_r = false, eq_d = false;
        if (valid) {
            const int r = (int)(i / p.g.cols), c = (int)(i - (long long)r * p.g.cols);
            col = p.s[i];
            const int cr = c + 1 < p.g.cols ? c + 1 : (p.g.periodic ? 0 : -1);
            const int rd = r + 1 < p.g.rows ? r + 1 : (p.g.periodic ? 0 : -1);
            eq_r = cr >= 0 && p.s[(long long)r * p.g.cols + cr] == col;
            eq_d = rd >= 0 && p.s[(long long)rd * p.g.cols + c] == col;
        }
        acc[0] += (unsigned long long)(__popcll(__ballot(eq_r)) + __popcll(__ballot(eq_d)));
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

// ---------------------------------------------------------------- Swendsen-Wang steps (PottsBonds, root_colour: potts_kern_dev.h)
using Item = SwItem<PottsBonds>;
using Params = SwParams<PottsBonds>;

// Rec: always empty (the Potts handle keeps no cluster-size records); the pack is there because sw_host.h names a measured
// instantiation of every one-workgroup kernel
template <class... Rec>
__global__ __launch_bounds__(kSwMaxThreads) void k10_sw_small(const Item* __restrict__ items, Item one, SwGeom g, int n_steps, int* err, Rec...) {
    extern __shared__ int s_lab[];
    __shared__ int s_bad;
    const Item& it = items ? items[blockIdx.x] : one;
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    const int rows = g.rows, cols = g.cols, periodic = g.pr;
    const int n = rows * cols, tid = threadIdx.x, nt = blockDim.x;
    int8_t* const s_spin = reinterpret_cast<int8_t*>(s_lab + n);
    if (tid == 0) s_bad = 0;
    for (int i = tid; i < n; i += nt) s_spin[i] = it.s[i];
    const int hc = (cols + 1) >> 1, npairs = rows * hc;
    for (int s = 0; s < n_steps; ++s) {
        const uint32_t t = it.k.t + (uint32_t)s;
        for (int i = tid; i < n; i += nt) s_lab[i] = i;
        __syncthreads();
        int budget = kBudget;
        for (int p = tid; p < npairs; p += nt) {
            const int r = p / hc, cp = p - r * hc;
            const u32x4 w = tsu_philox((uint32_t)cp, (uint32_t)r, t, it.k.tag_bond, it.k.k0, it.k.k1);
            const int rd = r + 1 < rows ? r + 1 : (periodic ? 0 : -1);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = 2 * cp + j;
                if (c >= cols) break;
                const int i = r * cols + c, si = s_spin[i];
                const int cr = c + 1 < cols ? c + 1 : (periodic ? 0 : -1);
                if (cr >= 0 && it.b.on(si, s_spin[r * cols + cr], j ? w.z : w.x))
                    if (!uf_union<false, WG>(s_lab, i, r * cols + cr, budget)) s_bad = 1;
                if (rd >= 0 && it.b.on(si, s_spin[rd * cols + c], j ? w.w : w.y))
                    if (!uf_union<false, WG>(s_lab, i, rd * cols + c, budget)) s_bad = 1;
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

__global__ __launch_bounds__(kLocalThreads) void k10_sw_local(Params p) {
    extern __shared__ int s_lab[];
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    const int TH = p.g.tr, TW = p.g.tc, n = TH * TW;
    int8_t* const s_spin = reinterpret_cast<int8_t*>(s_lab + n);
    const int ty = (int)(blockIdx.x / (unsigned)p.g.nc), tx = (int)blockIdx.x - ty * p.g.nc;
    const int r0 = ty * TH, c0 = tx * TW;
    const int th = p.g.rows - r0 < TH ? p.g.rows - r0 : TH, tw = p.g.cols - c0 < TW ? p.g.cols - c0 : TW;
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += kLocalThreads) {
        const int lr = i / TW, lc = i - lr * TW;
        s_lab[i] = i;
        s_spin[i] = (lr < th && lc < tw) ? p.s[(long long)(r0 + lr) * p.g.pitch + c0 + lc] : (int8_t)-1;  // outside: no colour
    }
    __syncthreads();
    int budget = kBudget;
    bool bad = false;
    const int hw = TW >> 1;
    for (int q = tid; q < TH * hw; q += kLocalThreads) {
        const int lr = q / hw, lc0 = 2 * (q - lr * hw);
        if (lr >= th || lc0 >= tw) continue;
        const u32x4 w = tsu_philox((uint32_t)(c0 + lc0) >> 1, (uint32_t)(r0 + lr), p.k.t, p.k.tag_bond, p.k.k0, p.k.k1);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int lc = lc0 + j;
            if (lc >= tw) break;
            const int i = lr * TW + lc, si = s_spin[i];
            if (lc + 1 < tw && p.b.on(si, s_spin[i + 1], j ? w.z : w.x)) bad |= !uf_union<false, WG>(s_lab, i, i + 1, budget);
            if (lr + 1 < th && p.b.on(si, s_spin[i + TW], j ? w.w : w.y)) bad |= !uf_union<false, WG>(s_lab, i, i + TW, budget);
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += kLocalThreads) {
        const int lr = i / TW, lc = i - lr * TW;
        if (lr >= th || lc >= tw) continue;
        budget = kBudget;
        const int root = uf_find<false, WG>(s_lab, i, budget);
        bad |= budget < 0;
        const int rr = root / TW, rc = root - rr * TW;
        p.labels[(long long)(r0 + lr) * p.g.cols + c0 + lc] = (r0 + rr) * p.g.cols + c0 + rc;
    }
    if (bad) raise_err(p.err);
}

// one lane per bond across a tile edge or the wrap (sw_seam)
__global__ __launch_bounds__(256) void k10_sw_merge(Params p) {
    int r, c, r2, c2;
    const int axis = sw_seam<2>(p.g, (long long)blockIdx.x * 256 + threadIdx.x, r, c, r2, c2);
    if (axis < 0) return;
    const int sa = p.s[(long long)r * p.g.pitch + c], sb = p.s[(long long)r2 * p.g.pitch + c2];
    if (!PottsBonds::sat(sa, sb)) return;
    const u32x4 w = tsu_philox((uint32_t)c >> 1, (uint32_t)r, p.k.t, p.k.tag_bond, p.k.k0, p.k.k1);
    const uint32_t u = axis ? ((c & 1) ? w.w : w.y) : ((c & 1) ? w.z : w.x);
    if ((uint64_t)u >= p.b.thr) return;
    int budget = kBudget;
    const int a = p.labels[(long long)r * p.g.cols + c], b = p.labels[(long long)r2 * p.g.cols + c2];
    if (!uf_union<false, __HIP_MEMORY_SCOPE_AGENT>(p.labels, a, b, budget)) raise_err(p.err);
}

// one lane per 4 sites of a row: the root of each site (labels only: no lane reads a colour another lane writes), the root's colour
// (one Philox block per distinct root of the lane), the colour stored as a byte
__global__ __launch_bounds__(256) void k10_sw_resolve(Params p, int quads) {
    const SwGeom& g = p.g;
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    const int r = (int)(lane / quads);
    const int c0 = 4 * (int)(lane - (long long)r * quads);
    if (r >= g.rows) return;
    int last = -1, last_colour = 0;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (c0 + j >= g.cols) break;
        const long long i = (long long)r * g.cols + c0 + j;
        const int x = sw_chase<false>(p.labels, p.labels[i], bad);
        if (x != last) {
            const int rr = x / g.cols, rc = x - rr * g.cols;
            last = x;
            last_colour = root_colour(rr, rc, p.b.q, p.k.t, p.k.tag_flip, p.k.k0, p.k.k1);
        }
        p.s[(long long)r * g.pitch + c0 + j] = (int8_t)last_colour;
    }
    if (bad) raise_err(p.err);
}

uint64_t threshold(double J, double T) {
    const double p = -expm1(-J / T);
    return (uint64_t)floor(p * 4294967296.0);
}

int tile_switch() {
    const char* e = getenv("TSU_SW_TILE");
    return e ? atoi(e) : 0;
}

int check_err(tsu_potts2d* L) {
    if (L->h_err && *L->h_err) {
        *L->h_err = 0;
        return tsu_fail(L->ctx, TSU_E_HIP, "potts2d: a cluster kernel's union / find loop hit its iteration cap; results invalid");
    }
    return TSU_OK;
}

struct K10 {
    static constexpr int DIM = 2;
    using Lattice = tsu_potts2d;
    using Bonds = PottsBonds;
    struct Model {
        double T;
    };
    static constexpr const char* who = "potts2d_cluster";
    [[maybe_unused]] static constexpr bool refuse_twice = false;  // no batch entry point
    static constexpr auto small = k10_sw_small<>;
    static constexpr auto small_measured = k10_sw_small<SwRecOut>;  // never launched: sw.measure stays 0
    static constexpr auto local = k10_sw_local;
    static constexpr auto merge = k10_sw_merge;
    static constexpr auto resolve = k10_sw_resolve;

    static int check_model(Lattice* L, const Model& m) {
        tsu_ctx* ctx = L->ctx;
        TSU_REQUIRE(ctx, isfinite(m.T) && m.T > 0.0, "Temperature must be positive");
        if (!(L->J > 0.0)) return tsu_fail(ctx, TSU_E_UNSUPPORTED, "potts2d_cluster: Swendsen-Wang steps need J > 0 (heat-bath sweeps take J <= 0)");
        for (int c = 0; c < L->q; ++c)
            if (L->h[c] != 0.0) return tsu_fail(ctx, TSU_E_UNSUPPORTED, "potts2d_cluster: Swendsen-Wang steps need a zero field");
        return TSU_OK;
    }
    static int check_err(Lattice* L) { return ::check_err(L); }
    static SwGeom geom(const Lattice* L) {
        SwGeom g = {};
        g.pitch = (long long)L->cols;
        g.depth = 1;
        g.rows = L->rows;
        g.cols = L->cols;
        g.pr = g.pc = L->periodic;
        return g;
    }
    static int8_t* spins(const Lattice* L) { return L->d_s; }
    static Bonds bonds(const Lattice* L, const Model& m) { return Bonds{threshold(L->J, m.T), L->q}; }
    static bool tile_forced() { return tile_switch() != 0; }
    static int tile(Lattice* L, SwGeom& g) {
        tsu_ctx* ctx = L->ctx;
        int edge = tile_switch();
        if (edge <= 0) edge = kTile;
        TSU_REQUIRE(ctx, edge >= 2 && edge <= 64 && (edge & 1) == 0, "TSU_SW_TILE must be an even edge in [2, 64] (got %d)", edge);
        g.tz = 1;
        g.tr = g.tc = edge;
        return TSU_OK;
    }
    static int local_threads(const SwGeom&) { return kLocalThreads; }
    static int grow_labels(Lattice* L, size_t bytes) {
        TSU_HIP_TRY(L->ctx, ising2d_grow(L->sw.d_labels, L->sw.labels_cap, bytes));
        return TSU_OK;
    }
};

// ---------------------------------------------------------------- host side of the heat bath and the observables
bool small_switch_off() {  // TSU_POTTS_SMALL=0 (tests, read per call): every lattice on k10_sweep
    const char* e = getenv("TSU_POTTS_SMALL");
    return e && atoi(e) == 0;
}

bool hb_small_route(const tsu_potts2d* L) { return !small_switch_off() && (long long)L->rows * L->cols <= kSmallSites; }

int hb_check(tsu_potts2d* L, double T, int n_sweeps, uint32_t replica, PottsTab* tab) {
    tsu_ctx* ctx = L->ctx;
    const char* why = potts_tables(L->q, L->J, L->h, T, tab);
    TSU_REQUIRE(ctx, !why, "potts2d_sweep: %s", why);
    TSU_REQUIRE(ctx, n_sweeps >= 0, "potts2d_sweep: n_sweeps must be >= 0");
    TSU_REQUIRE_REPLICA(ctx, replica, "potts2d_sweep");
    return TSU_OK;
}

int hb_sweep(tsu_potts2d* L, const PottsTab& tab, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica) {
    tsu_ctx* ctx = L->ctx;
    if (n_sweeps == 0) return TSU_OK;
    PottsSweep p;
    p.s = L->d_s;
    p.g = PottsGeom{L->rows, L->cols, L->periodic};
    p.k = PottsKeys{(uint32_t)seed, (uint32_t)(seed >> 32), TSU_TAG_ISING_HI | (replica << 8), TSU_TAG_ISING_LO | (replica << 8)};
    p.t = tab;
    const long long lanes = (long long)L->rows * ((L->cols + 15) >> 4);
    if (hb_small_route(L)) {
        p.hs = sweep0;
        hipLaunchKernelGGL(k10_small, dim3(1), dim3((unsigned)sw_threads(lanes)), 0, ctx->stream, p, n_sweeps);
        L->launches += 1;
    } else {
        for (int k = 0; k < n_sweeps; ++k)
            for (uint32_t colour = 0; colour < 2; ++colour) {
                p.hs = 2u * (sweep0 + (uint32_t)k) + colour;  // 32-bit words: the header says so
                if ((L->cols & 15) == 0) hipLaunchKernelGGL(k10_sweep<true>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, ctx->stream, p);
                else hipLaunchKernelGGL(k10_sweep<false>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, ctx->stream, p);
                L->launches += 1;
            }
    }
    TSU_HIP_TRY(ctx, hipGetLastError());
    return TSU_OK;
}

int measure_into(tsu_potts2d* L, long long* d_row) {
    tsu_ctx* ctx = L->ctx;
    TSU_HIP_TRY(ctx, hipMemsetAsync(d_row, 0, TSU_POTTS_RECORD_WORDS * sizeof(long long), ctx->stream));
    PottsMeasure m = {L->d_s, PottsGeom{L->rows, L->cols, L->periodic}, L->q, (unsigned long long*)d_row};
    const long long n = (long long)L->rows * L->cols, want = (n + 255) / 256;
    hipLaunchKernelGGL(k10_measure, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(256), 0, ctx->stream, m);
    TSU_HIP_TRY(ctx, hipGetLastError());
    L->launches += 1;
    return TSU_OK;
}

}  // namespace

extern "C" {

int tsu_potts2d_check_model(int q, double J, const double* h, double T, double* tables) {
    PottsTab t;
    if (potts_tables(q, J, h, T, &t)) return TSU_E_INVALID;
    if (tables) {
        for (int n = 0; n < 5; ++n) tables[n] = t.E[n];
        for (int c = 0; c < TSU_POTTS_MAX_Q; ++c) tables[5 + c] = t.F[c];
    }
    return TSU_OK;
}

int tsu_potts2d_cluster_threshold(double J, double T, uint64_t* thr) {
    if (!thr || !(T > 0.0) || !isfinite(T) || !isfinite(J) || !(J > 0.0)) return TSU_E_INVALID;
    *thr = threshold(J, T);
    return TSU_OK;
}

int tsu_potts2d_create(tsu_ctx* ctx, int rows, int cols, int q, int periodic, tsu_potts2d** out) {
    TSU_ENTER(ctx);
    if (!ctx || !out) return TSU_E_INVALID;
    TSU_REQUIRE(ctx, q >= 2 && q <= TSU_POTTS_MAX_Q, "potts2d_create: q must be in 2 .. 8 (got %d)", q);
    TSU_REQUIRE(ctx, rows >= 1 && cols >= 1, "potts2d_create: rows and cols must be >= 1");
    TSU_REQUIRE(ctx, (long long)rows * cols < (1ll << 31), "potts2d_create: %lld sites exceed 32-bit labels", (long long)rows * cols);
    TSU_REQUIRE(ctx, !periodic || ((rows & 1) == 0 && (cols & 1) == 0), "potts2d_create: a periodic lattice needs even rows and cols");
    tsu_potts2d* L = new tsu_potts2d();
    L->ctx = ctx;
    L->rows = rows;
    L->cols = cols;
    L->q = q;
    L->periodic = periodic != 0;
    L->J = 1.0;
    const size_t n = (size_t)rows * cols;
    hipError_t e = hipMalloc((void**)&L->d_s, n);
    if (e == hipSuccess) e = hipMalloc((void**)&L->d_obs, TSU_POTTS_RECORD_WORDS * sizeof(long long));
    if (e == hipSuccess) e = hipMemsetAsync(L->d_s, 0, n, ctx->stream);
    if (e != hipSuccess) {
        if (L->d_s) (void)hipFree(L->d_s);
        if (L->d_obs) (void)hipFree(L->d_obs);
        delete L;
        return tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "potts2d_create: %s", hipGetErrorString(e));
    }
    *out = L;
    return TSU_OK;
}

int tsu_potts2d_destroy(tsu_potts2d* L) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    (void)hipStreamSynchronize(L->ctx->stream);
    (void)hipFree(L->d_s);
    (void)hipFree(L->d_obs);
    if (L->d_rec) (void)hipFree(L->d_rec);
    if (L->h_err) (void)hipHostFree(L->h_err);
    tsu_sw_scratch_free(L->sw);
    delete L;
    return TSU_OK;
}

int tsu_potts2d_set_model(tsu_potts2d* L, double J, const double* h) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    TSU_REQUIRE(L->ctx, isfinite(J), "potts2d_set_model: J must be finite");
    for (int c = 0; h && c < L->q; ++c) TSU_REQUIRE(L->ctx, isfinite(h[c]), "potts2d_set_model: h must be finite");
    L->J = J;  // the bound on (4 |J| + max h - min h) / T is checked with every sweep's temperature
    for (int c = 0; c < TSU_POTTS_MAX_Q; ++c) L->h[c] = (h && c < L->q) ? h[c] : 0.0;
    return TSU_OK;
}

int tsu_potts2d_set_spins(tsu_potts2d* L, const int8_t* colours) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, colours, "potts2d_set_spins: colours is NULL");
    const size_t n = (size_t)L->rows * L->cols;
    for (size_t i = 0; i < n; ++i)
        TSU_REQUIRE(ctx, colours[i] >= 0 && colours[i] < L->q, "potts2d_set_spins: colour %d at site %zu is outside 0 .. %d", (int)colours[i], i, L->q - 1);
    TSU_HIP_TRY(ctx, hipMemcpyAsync(L->d_s, colours, n, hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int tsu_potts2d_get_spins(tsu_potts2d* L, int8_t* colours) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, colours, "potts2d_get_spins: colours is NULL");
    TSU_HIP_TRY(ctx, hipMemcpyAsync(colours, L->d_s, (size_t)L->rows * L->cols, hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return check_err(L);
}

int tsu_potts2d_fill(tsu_potts2d* L, int colour) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    TSU_REQUIRE(L->ctx, colour >= 0 && colour < L->q, "potts2d_fill: colour %d is outside 0 .. %d", colour, L->q - 1);
    TSU_HIP_TRY(L->ctx, hipMemsetAsync(L->d_s, colour, (size_t)L->rows * L->cols, L->ctx->stream));
    return TSU_OK;
}

int tsu_potts2d_sweep(tsu_potts2d* L, double T, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    PottsTab tab;
    const int rc = hb_check(L, T, n_sweeps, replica, &tab);
    if (rc != TSU_OK) return rc;
    return hb_sweep(L, tab, n_sweeps, seed, sweep0, replica);
}

int tsu_potts2d_cluster_sweep(tsu_potts2d* L, double T, int n_steps, uint64_t seed, uint32_t step0, uint32_t replica) {
    TSU_ENTER(L ? L->ctx : nullptr);
    return sw_sweep<K10>(L, K10::Model{T}, n_steps, seed, step0, replica);
}

int tsu_potts2d_route(tsu_potts2d* L, int algorithm, int* route) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L || !route) return TSU_E_INVALID;
    TSU_REQUIRE(L->ctx, algorithm == TSU_POTTS_HEAT_BATH || algorithm == TSU_POTTS_SWENDSEN_WANG, "potts2d_route: unknown algorithm %d", algorithm);
    if (algorithm == TSU_POTTS_HEAT_BATH) *route = hb_small_route(L) ? TSU_POTTS_ROUTE_SMALL : TSU_POTTS_ROUTE_SWEEP;
    else *route = sw_small_route<K10>(L) ? TSU_POTTS_ROUTE_SW_SMALL : TSU_POTTS_ROUTE_SW_TILES;
    return TSU_OK;
}

int tsu_potts2d_measure(tsu_potts2d* L, int64_t* row) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, row, "potts2d_measure: row is NULL");
    const int rc = measure_into(L, L->d_obs);
    if (rc != TSU_OK) return rc;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(row, L->d_obs, TSU_POTTS_RECORD_WORDS * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return check_err(L);
}

int tsu_potts2d_run(tsu_potts2d* L, double T, int n_meas, int sweeps_between, int algorithm, uint64_t seed, uint32_t counter0,
                    uint32_t replica) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, algorithm == TSU_POTTS_HEAT_BATH || algorithm == TSU_POTTS_SWENDSEN_WANG, "potts2d_run: unknown algorithm %d", algorithm);
    TSU_REQUIRE(ctx, n_meas >= 0 && sweeps_between >= 0, "potts2d_run: n_meas and sweeps_between must be >= 0");
    const long long total = (long long)n_meas * sweeps_between;
    TSU_REQUIRE(ctx, total <= (1ll << 31), "potts2d_run: %lld updates exceed one call", total);
    PottsTab tab;
    int rc;
    if (algorithm == TSU_POTTS_HEAT_BATH) {
        rc = hb_check(L, T, sweeps_between, replica, &tab);
    } else {
        rc = sw_check_call<K10>(L, K10::Model{T}, 0, counter0, replica);
    }
    if (rc != TSU_OK) return rc;
    TSU_REQUIRE(ctx, algorithm == TSU_POTTS_HEAT_BATH || (uint64_t)counter0 + (uint64_t)total <= (1ull << 32), "potts2d_run: step counter overflow");
    const size_t bytes = (size_t)n_meas * TSU_POTTS_RECORD_WORDS * sizeof(long long);
    TSU_HIP_TRY(ctx, ising2d_grow(L->d_rec, L->rec_cap, bytes ? bytes : sizeof(long long)));
    L->rec_rows = 0;
    for (int k = 0; k < n_meas; ++k) {
        const uint32_t c0 = counter0 + (uint32_t)((long long)k * sweeps_between);
        rc = algorithm == TSU_POTTS_HEAT_BATH ? hb_sweep(L, tab, sweeps_between, seed, c0, replica)
                                              : sw_sweep<K10>(L, K10::Model{T}, sweeps_between, seed, c0, replica);
        if (rc == TSU_OK) rc = measure_into(L, L->d_rec + (size_t)k * TSU_POTTS_RECORD_WORDS);
        if (rc != TSU_OK) return rc;
        L->rec_rows = k + 1;
    }
    return TSU_OK;
}

int tsu_potts2d_record(tsu_potts2d* L, int64_t* rows, int max_rows, int* n_rows) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, n_rows && max_rows >= 0 && (rows || max_rows == 0), "potts2d_record: n_rows is NULL, max_rows negative or rows NULL");
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const int rc = check_err(L);
    if (rc != TSU_OK) return rc;
    *n_rows = L->rec_rows;
    const int n = L->rec_rows < max_rows ? L->rec_rows : max_rows;
    if (n > 0) TSU_HIP_TRY(ctx, hipMemcpy(rows, L->d_rec, (size_t)n * TSU_POTTS_RECORD_WORDS * sizeof(int64_t), hipMemcpyDeviceToHost));
    return TSU_OK;
}

int tsu_potts2d_launch_count(tsu_potts2d* L, uint64_t* n) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L || !n) return TSU_E_INVALID;
    *n = L->launches + L->sw.launches;
    return TSU_OK;
}

}  // extern "C"

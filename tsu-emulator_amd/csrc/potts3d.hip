// potts3d.hip -- K10 in 3-D: q-state Potts lattices on the cubic lattice, on a handle of their own (gfx950): heat-bath sweeps,
// Swendsen-Wang steps and exact integer observables (include/tsu_hip_potts3d.h; the contracts are DESIGN.md section 3).
//
// A D x R x C lattice of int8 colours, row-major, pitch = cols, no pad; global row rho = z R + r, site index i = rho C + c, one
// periodic flag per axis.  Everything that draws a random word takes K10's 2-D counters with rho in place of r, as K8 does with
// K7's, so a one-layer lattice (1, R, C) with periodic (0, p, p) takes potts2d.hip's colours bit for bit on every route.
//
// Heat bath, half-sweep hs = 2 sweep + colour, colour = (z + r + c) & 1.  One Philox block serves the 8 same-colour sites of an
// octet (16 consecutive columns of a global row); the rule is potts_dev.h's with up to six neighbours (PottsTab6, potts_cum6), the
// lo16 block drawn only by an octet with a site whose colour differs between lo16 = 0 and lo16 = 65535.
//   k10_3d_small   a lattice of at most 16384 sites in one workgroup's LDS for all sweeps of a call, a barrier per half-sweep
//   k10_3d_sweep   one launch per half-sweep through HBM, one lane per octet.  Rows of whole octets (cols % 16 == 0): the row, the
//                  rows above and below and the two layers by aligned 16-byte loads (five loads and one edge byte), one 16-byte
//                  store; any other width: bounds-checked byte loads
// Swendsen-Wang steps: K8's tile geometry, seams (sw_seam<3>) and layer-bond word with K10's bond policy (two equal colours and
// u < floor(-expm1(-J / T) 2^32)) and root colour ((uint64)W q) >> 32, driven through sw_host.h by the traits struct K10x3 below.
//   k10_3d_sw_small   at most 16384 sites, all steps of a call in one launch
//   k10_3d_sw_local / k10_3d_sw_merge / k10_3d_sw_resolve   on tz x tr x tc tiles, agent-scope atomicMin on the seams
// k10_3d_measure: n_eq over three axes and N_0 .. N_7 by wave ballots, one LDS atomic per wave and word, one global atomic per
// workgroup and word.
#include <math.h>
#include <stdlib.h>

#include "potts_dev.h"
#include "potts_kern_dev.h"
#include "sw_host.h"

struct tsu_potts3d {
    tsu_ctx* ctx;
    int depth, rows, cols, q;
    int pz, pr, pc;
    int8_t* d_s;  // depth * rows * cols colours, pitch = cols
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

constexpr int kSmallSites = 16384;

struct Potts3Geom {
    int depth, rows, cols;
    int pz, pr, pc;
};

struct Potts3Sweep {
    int8_t* s;
    Potts3Geom g;
    PottsKeys k;
    uint32_t hs;  // k10_3d_sweep: the half-sweep; k10_3d_small: the first sweep of the call
    PottsTab6 t;
};

// Site m of the octet (rho, o) with the neighbour colours zm, zp, up, dn, lf, rt (-1: none): its new colour
__device__ __forceinline__ int potts_site6(const PottsTab6& t, const PottsKeys& k, uint32_t hs, int rho, int o, int m, int zm, int zp, int up,
                                           int dn, int lf, int rt, PottsDraw& d) {
    double Z[TSU_POTTS_MAX_Q];
    potts_cum6(t, zm, zp, up, dn, lf, rt, Z);
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

// the global rows of the four neighbour rows of (z, r): above and below in the layer, the same row of the layers below and above
// (-1: none)
struct Potts3Rows {
    int ru, rd, rzm, rzp;
};

__device__ __forceinline__ Potts3Rows potts3_rows(const Potts3Geom& g, int z, int r) {
    const int rho = z * g.rows + r;
    Potts3Rows n;
    n.ru = r > 0 ? rho - 1 : (g.pr ? rho + g.rows - 1 : -1);
    n.rd = r + 1 < g.rows ? rho + 1 : (g.pr ? rho - r : -1);
    n.rzm = z > 0 ? rho - g.rows : (g.pz ? (g.depth - 1) * g.rows + r : -1);
    n.rzp = z + 1 < g.depth ? rho + g.rows : (g.pz ? r : -1);
    return n;
}

// One colour of the octet (rho, o): sites c = 16 o + 2 m + par, m = 0 .. 7.  s: the lattice in HBM or LDS, pitch = cols.  The sites
// written have this half-sweep's colour, the sites read the other one.  Every index stays inside [0, depth rows cols)
__device__ __forceinline__ void potts3_octet(int8_t* s, const Potts3Geom& g, const PottsTab6& t, const PottsKeys& k, uint32_t hs, int rho,
                                             int o, int colour) {
    const int z = rho / g.rows, r = rho - z * g.rows;
    const int par = (z + r + colour) & 1, c0 = 16 * o;
    const Potts3Rows nb = potts3_rows(g, z, r);
    const long long row = (long long)rho * g.cols;
    PottsDraw d = potts_draw(k, hs, rho, o);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int c = c0 + 2 * m + par;
        if (c >= g.cols) break;
        const int cl = c > 0 ? c - 1 : (g.pc ? g.cols - 1 : -1);
        const int cr = c + 1 < g.cols ? c + 1 : (g.pc ? 0 : -1);
        const int zm = nb.rzm >= 0 ? s[(long long)nb.rzm * g.cols + c] : -1, zp = nb.rzp >= 0 ? s[(long long)nb.rzp * g.cols + c] : -1;
        const int up = nb.ru >= 0 ? s[(long long)nb.ru * g.cols + c] : -1, dn = nb.rd >= 0 ? s[(long long)nb.rd * g.cols + c] : -1;
        const int lf = cl >= 0 ? s[row + cl] : -1, rt = cr >= 0 ? s[row + cr] : -1;
        s[row + c] = (int8_t)potts_site6(t, k, hs, rho, o, m, zm, zp, up, dn, lf, rt, d);
    }
}

// The same half-sweep of an octet of a lattice whose rows are whole octets (cols % 16 == 0, so every 16-byte row segment is aligned
// and holds sites only): five 16-byte loads and one edge byte, one 16-byte store (the other colour's bytes go back as read; nobody
// writes them in this launch).  PAR = the parity of the colour's columns in this row
template <int PAR>
__device__ __forceinline__ void potts3_octet_rows16(int8_t* s, const Potts3Geom& g, const PottsTab6& t, const PottsKeys& k, uint32_t hs, int z,
                                                    int r, int o) {
    const int c0 = 16 * o, rho = z * g.rows + r;
    const Potts3Rows nb = potts3_rows(g, z, r);
    const long long row = (long long)rho * g.cols;
    const uint4 C = *reinterpret_cast<const uint4*>(s + row + c0);
    // a missing row or layer is loaded from this row (a valid address, no branch); what it brings is never used
    const uint4 U = *reinterpret_cast<const uint4*>(s + (long long)(nb.ru >= 0 ? nb.ru : rho) * g.cols + c0);
    const uint4 D = *reinterpret_cast<const uint4*>(s + (long long)(nb.rd >= 0 ? nb.rd : rho) * g.cols + c0);
    const uint4 A = *reinterpret_cast<const uint4*>(s + (long long)(nb.rzm >= 0 ? nb.rzm : rho) * g.cols + c0);
    const uint4 B = *reinterpret_cast<const uint4*>(s + (long long)(nb.rzp >= 0 ? nb.rzp : rho) * g.cols + c0);
    // the one neighbour outside the 16 bytes: left of position 0 (PAR = 0) or right of position 15 (PAR = 1)
    const int ce = PAR == 0 ? (c0 > 0 ? c0 - 1 : (g.pc ? g.cols - 1 : -1)) : (c0 + 16 < g.cols ? c0 + 16 : (g.pc ? 0 : -1));
    const int s_edge = ce >= 0 ? (int)s[row + ce] : -1;
    PottsDraw d = potts_draw(k, hs, rho, o);
    uint32_t o0 = C.x, o1 = C.y, o2 = C.z, o3 = C.w;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int i = 2 * m + PAR;
        const int zm = nb.rzm >= 0 ? colour_at(A, i) : -1, zp = nb.rzp >= 0 ? colour_at(B, i) : -1;
        const int up = nb.ru >= 0 ? colour_at(U, i) : -1, dn = nb.rd >= 0 ? colour_at(D, i) : -1;
        const int lf = i > 0 ? colour_at(C, i - 1) : s_edge, rt = i < 15 ? colour_at(C, i + 1) : s_edge;
        const uint32_t col = (uint32_t)potts_site6(t, k, hs, rho, o, m, zm, zp, up, dn, lf, rt, d);
        const int sh = 8 * (i & 3);
        uint32_t& w = (i >> 2) == 0 ? o0 : ((i >> 2) == 1 ? o1 : ((i >> 2) == 2 ? o2 : o3));
        w = (w & ~(0xFFu << sh)) | (col << sh);
    }
    *reinterpret_cast<uint4*>(s + row + c0) = make_uint4(o0, o1, o2, o3);
}

// ROWS16: the lattice's rows are whole octets (the host's choice; two instantiations, so that neither carries the other's registers)
template <bool ROWS16>
__global__ __launch_bounds__(256) void k10_3d_sweep(Potts3Sweep p) {
    const int noct = (p.g.cols + 15) >> 4;
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= (long long)p.g.depth * p.g.rows * noct) return;
    const int rho = (int)(lane / noct), o = (int)(lane - (long long)rho * noct);
    const int colour = (int)(p.hs & 1u);
    if constexpr (!ROWS16) {
        potts3_octet(p.s, p.g, p.t, p.k, p.hs, rho, o, colour);
    } else {
        const int z = rho / p.g.rows, r = rho - z * p.g.rows;
        if (((z + r + colour) & 1) == 0) potts3_octet_rows16<0>(p.s, p.g, p.t, p.k, p.hs, z, r, o);
        else potts3_octet_rows16<1>(p.s, p.g, p.t, p.k, p.hs, z, r, o);
    }
}

__global__ __launch_bounds__(kSwMaxThreads) void k10_3d_small(Potts3Sweep p, int n_sweeps) {
    __shared__ int8_t s_sp[kSmallSites];
    const int n = p.g.depth * p.g.rows * p.g.cols, tid = threadIdx.x, nt = blockDim.x;  // n <= kSmallSites: the host's route
    const int noct = (p.g.cols + 15) >> 4, nlanes = p.g.depth * p.g.rows * noct;
    for (int i = tid; i < n; i += nt) s_sp[i] = p.s[i];
    __syncthreads();
    for (int s = 0; s < n_sweeps; ++s) {
#pragma unroll 1
        for (int colour = 0; colour < 2; ++colour) {
            const uint32_t hs = 2u * (p.hs + (uint32_t)s) + (uint32_t)colour;
            for (int l = tid; l < nlanes; l += nt) {
                const int rho = l / noct, o = l - rho * noct;
                potts3_octet(s_sp, p.g, p.t, p.k, hs, rho, o, colour);
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < n; i += nt) p.s[i] = s_sp[i];
}

// ---------------------------------------------------------------- observables
struct Potts3Measure {
    const int8_t* s;
    Potts3Geom g;
    int q;
    unsigned long long* row;  // 9 words, zeroed on the stream ahead of the launch
};

__global__ __launch_bounds__(256) void k10_3d_measure(Potts3Measure p) {
    __shared__ unsigned long long s_row[TSU_POTTS_RECORD_WORDS];
    if (threadIdx.x < TSU_POTTS_RECORD_WORDS) s_row[threadIdx.x] = 0;
    __syncthreads();
    const long long plane = (long long)p.g.rows * p.g.cols, n = plane * p.g.depth;
    unsigned long long acc[TSU_POTTS_RECORD_WORDS] = {};  // wave-uniform: every lane of a wave holds the wave's counts
    for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {  // whole waves stay in
        const long long i = base + threadIdx.x;
        const bool valid = i < n;
        int col = -1;
        bool eq_r = false, eq_d = false, eq_l = false;
        if (valid) {
            const int z = (int)(i / plane);
            const long long rem = i - (long long)z * plane;
            const int r = (int)(rem / p.g.cols), c = (int)(rem - (long long)r * p.g.cols);
            col = p.s[i];
            const int cr = c + 1 < p.g.cols ? c + 1 : (p.g.pc ? 0 : -1);
            const int rd = r + 1 < p.g.rows ? r + 1 : (p.g.pr ? 0 : -1);
            const int zl = z + 1 < p.g.depth ? z + 1 : (p.g.pz ? 0 : -1);
            eq_r = cr >= 0 && p.s[i - c + cr] == col;
            eq_d = rd >= 0 && p.s[(long long)z * plane + (long long)rd * p.g.cols + c] == col;
            eq_l = zl >= 0 && p.s[(long long)zl * plane + rem] == col;
        }
        acc[0] += (unsigned long long)(__popcll(__ballot(eq_r)) + __popcll(__ballot(eq_d)) + __popcll(__ballot(eq_l)));
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
// instantiation of every one-workgroup kernel.  LDS: 4 B labels + 1 B colours a site (the host's dynamic size), n <= 16384
template <class... Rec>
__global__ __launch_bounds__(kSwMaxThreads) void k10_3d_sw_small(const Item* __restrict__ items, Item one, SwGeom g, int n_steps, int* err, Rec...) {
    extern __shared__ int s_lab[];
    __shared__ int s_bad;
    const Item& it = items ? items[blockIdx.x] : one;
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    const int depth = g.depth, rows = g.rows, cols = g.cols, pz = g.pz, pr = g.pr, pc = g.pc;
    const int nrows = depth * rows, n = nrows * cols, tid = threadIdx.x, nt = blockDim.x;
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
            const int z = rho / rows, r = rho - z * rows;
            const u32x4 w = tsu_philox((uint32_t)cp, (uint32_t)rho, t, it.k.tag_bond, it.k.k0, it.k.k1);
            const int rd = r + 1 < rows ? rho + 1 : (pr ? z * rows : -1);  // global row of the down neighbour
            const int rf = z + 1 < depth ? rho + rows : (pz ? r : -1);     // ... of the layer neighbour
            u32x4 wl = {0u, 0u, 0u, 0u};  // the layer bonds' block, drawn once a site of the pair has a layer neighbour of its colour
            bool have_wl = false;
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
                if (rf >= 0 && PottsBonds::sat(si, s_spin[rf * cols + c])) {
                    if (!have_wl) wl = tsu_philox((uint32_t)cp >> 1, (uint32_t)rho, t, it.k.tag_layer, it.k.k0, it.k.k1);
                    have_wl = true;
                    if ((uint64_t)word_of(wl, c & 3) < it.b.thr)
                        if (!uf_union<false, WG>(s_lab, i, rf * cols + c, budget)) s_bad = 1;
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

// tile blockIdx.x (row-major over nz x nr x nc) of tz x tr x tc sites; bonds with both ends in the tile, none across its faces or a
// wrap.  LDS: tz*tr*tc int32 labels (tile-local, row-major: the same order as the global indices inside a tile) and as many colours.
// Writes the global index of every site's tile root
__global__ __launch_bounds__(kSwMaxThreads) void k10_3d_sw_local(Params p) {
    extern __shared__ int s_lab[];
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    const int TZ = p.g.tz, TR = p.g.tr, TC = p.g.tc, n = TZ * TR * TC;
    int8_t* const s_spin = reinterpret_cast<int8_t*>(s_lab + n);
    const int bz = (int)(blockIdx.x / (unsigned)(p.g.nr * p.g.nc)), brc = (int)blockIdx.x - bz * p.g.nr * p.g.nc;
    const int br = brc / p.g.nc, bc = brc - br * p.g.nc;
    const int z0 = bz * TZ, r0 = br * TR, c0 = bc * TC;
    const int tz = p.g.depth - z0 < TZ ? p.g.depth - z0 : TZ, tr = p.g.rows - r0 < TR ? p.g.rows - r0 : TR, tc = p.g.cols - c0 < TC ? p.g.cols - c0 : TC;
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int i = tid; i < n; i += nt) {
        const int lz = i / (TR * TC), rem = i - lz * TR * TC, lr = rem / TC, lc = rem - lr * TC;
        s_lab[i] = i;
        s_spin[i] = (lz < tz && lr < tr && lc < tc) ? p.s[((long long)(z0 + lz) * p.g.rows + r0 + lr) * p.g.pitch + c0 + lc] : (int8_t)-1;  // outside: no colour
    }
    __syncthreads();
    int budget = kBudget;
    bool bad = false;
    const int hw = TC >> 1;
    for (int q = tid; q < TZ * TR * hw; q += nt) {
        const int lz = q / (TR * hw), rem = q - lz * TR * hw, lr = rem / hw, lc0 = 2 * (rem - lr * hw);
        if (lz >= tz || lr >= tr || lc0 >= tc) continue;
        const long long rho = (long long)(z0 + lz) * p.g.rows + r0 + lr;
        const u32x4 w = tsu_philox((uint32_t)(c0 + lc0) >> 1, (uint32_t)rho, p.k.t, p.k.tag_bond, p.k.k0, p.k.k1);
        u32x4 wl = {0u, 0u, 0u, 0u};
        bool have_wl = false;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int lc = lc0 + j;
            if (lc >= tc) break;
            const int i = (lz * TR + lr) * TC + lc, si = s_spin[i];
            if (lc + 1 < tc && p.b.on(si, s_spin[i + 1], j ? w.z : w.x)) bad |= !uf_union<false, WG>(s_lab, i, i + 1, budget);
            if (lr + 1 < tr && p.b.on(si, s_spin[i + TC], j ? w.w : w.y)) bad |= !uf_union<false, WG>(s_lab, i, i + TC, budget);
            if (lz + 1 < tz && PottsBonds::sat(si, s_spin[i + TR * TC])) {
                if (!have_wl) wl = tsu_philox((uint32_t)(c0 + lc0) >> 2, (uint32_t)rho, p.k.t, p.k.tag_layer, p.k.k0, p.k.k1);
                have_wl = true;
                if ((uint64_t)word_of(wl, (c0 + lc) & 3) < p.b.thr) bad |= !uf_union<false, WG>(s_lab, i, i + TR * TC, budget);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += nt) {
        const int lz = i / (TR * TC), rem = i - lz * TR * TC, lr = rem / TC, lc = rem - lr * TC;
        if (lz >= tz || lr >= tr || lc >= tc) continue;
        budget = kBudget;
        const int root = uf_find<false, WG>(s_lab, i, budget);
        bad |= budget < 0;
        const int rz = root / (TR * TC), rrem = root - rz * TR * TC, rr = rrem / TC, rc = rrem - rr * TC;
        p.labels[((long long)(z0 + lz) * p.g.rows + r0 + lr) * p.g.cols + c0 + lc] = ((z0 + rz) * p.g.rows + r0 + rr) * p.g.cols + c0 + rc;
    }
    if (bad) raise_err(p.err);
}

// one lane per bond across a tile face or a wrap (sw_seam: column seams, row seams, layer seams)
__global__ __launch_bounds__(256) void k10_3d_sw_merge(Params p) {
    long long rho, rho2;
    int c, c2;
    const int axis = sw_seam<3>(p.g, (long long)blockIdx.x * 256 + threadIdx.x, rho, c, rho2, c2);
    if (axis < 0) return;
    const int sa = p.s[rho * p.g.pitch + c], sb = p.s[rho2 * p.g.pitch + c2];
    if (!PottsBonds::sat(sa, sb)) return;
    uint32_t u;
    if (axis == 2) {
        u = word_of(tsu_philox((uint32_t)c >> 2, (uint32_t)rho, p.k.t, p.k.tag_layer, p.k.k0, p.k.k1), c & 3);
    } else {
        u = word_of(tsu_philox((uint32_t)c >> 1, (uint32_t)rho, p.k.t, p.k.tag_bond, p.k.k0, p.k.k1), 2 * (c & 1) + axis);
    }
    if ((uint64_t)u >= p.b.thr) return;
    int budget = kBudget;
    const int a = p.labels[rho * p.g.cols + c], b = p.labels[rho2 * p.g.cols + c2];
    if (!uf_union<false, __HIP_MEMORY_SCOPE_AGENT>(p.labels, a, b, budget)) raise_err(p.err);
}

// one lane per 4 sites of a global row: the root of each site (labels only: no lane reads a colour another lane writes), the root's
// colour (one Philox block per distinct root of the lane), the colour stored as a byte
__global__ __launch_bounds__(256) void k10_3d_sw_resolve(Params p, int quads) {
    const SwGeom& g = p.g;
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long rho = lane / quads;
    const int c0 = 4 * (int)(lane - rho * quads);
    if (rho >= (long long)g.depth * g.rows) return;
    int last = -1, last_colour = 0;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (c0 + j >= g.cols) break;
        const int x = sw_chase<false>(p.labels, p.labels[rho * g.cols + c0 + j], bad);
        if (x != last) {
            const int rr = x / g.cols, rc = x - rr * g.cols;
            last = x;
            last_colour = root_colour(rr, rc, p.b.q, p.k.t, p.k.tag_flip, p.k.k0, p.k.k1);
        }
        p.s[rho * g.pitch + c0 + j] = (int8_t)last_colour;
    }
    if (bad) raise_err(p.err);
}

int check_err(tsu_potts3d* L) {
    if (L->h_err && *L->h_err) {
        *L->h_err = 0;
        return tsu_fail(L->ctx, TSU_E_HIP, "potts3d: a cluster kernel's union / find loop hit its iteration cap; results invalid");
    }
    return TSU_OK;
}

long long sites_of(const tsu_potts3d* L) { return (long long)L->depth * L->rows * L->cols; }

struct K10x3 {
    static constexpr int DIM = 3;
    using Lattice = tsu_potts3d;
    using Bonds = PottsBonds;
    struct Model {
        double T;
    };
    static constexpr const char* who = "potts3d_cluster";
    [[maybe_unused]] static constexpr bool refuse_twice = false;  // no batch entry point
    static constexpr auto small = k10_3d_sw_small<>;
    static constexpr auto small_measured = k10_3d_sw_small<SwRecOut>;  // never launched: sw.measure stays 0
    static constexpr auto local = k10_3d_sw_local;
    static constexpr auto merge = k10_3d_sw_merge;
    static constexpr auto resolve = k10_3d_sw_resolve;

    static int check_model(Lattice* L, const Model& m) {
        tsu_ctx* ctx = L->ctx;
        TSU_REQUIRE(ctx, isfinite(m.T) && m.T > 0.0, "Temperature must be positive");
        if (!(L->J > 0.0)) return tsu_fail(ctx, TSU_E_UNSUPPORTED, "potts3d_cluster: Swendsen-Wang steps need J > 0 (heat-bath sweeps take J <= 0)");
        for (int c = 0; c < L->q; ++c)
            if (L->h[c] != 0.0) return tsu_fail(ctx, TSU_E_UNSUPPORTED, "potts3d_cluster: Swendsen-Wang steps need a zero field");
        return TSU_OK;
    }
    static int check_err(Lattice* L) { return ::check_err(L); }
    static SwGeom geom(const Lattice* L) {
        SwGeom g = {};
        g.pitch = (long long)L->cols;
        g.depth = L->depth;
        g.rows = L->rows;
        g.cols = L->cols;
        g.pz = L->pz;
        g.pr = L->pr;
        g.pc = L->pc;
        return g;
    }
    static int8_t* spins(const Lattice* L) { return L->d_s; }
    static Bonds bonds(const Lattice* L, const Model& m) {
        const double p = -expm1(-L->J / m.T);  // tsu_potts2d_cluster_threshold's expression
        return Bonds{(uint64_t)floor(p * 4294967296.0), L->q};
    }
    static bool tile_forced() { return sw3d_tile_forced(); }
    static int tile(Lattice* L, SwGeom& g) { return sw3d_tile(L->ctx, L->depth, L->rows, L->cols, g); }
    static int local_threads(const SwGeom& g) { return sw_threads((g.tz * g.tr * g.tc + 15) / 16); }
    static int grow_labels(Lattice* L, size_t bytes) {
        const hipError_t e = ising2d_grow(L->sw.d_labels, L->sw.labels_cap, bytes);
        if (e == hipSuccess) return TSU_OK;
        (void)hipGetLastError();
        return tsu_fail(L->ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "potts3d_cluster: the labels buffer: %s (%zu bytes)",
                        hipGetErrorString(e), bytes);
    }
};

// ---------------------------------------------------------------- host side of the heat bath and the observables
bool small_switch_off() {  // TSU_POTTS_SMALL=0 (tests, read per call): every lattice on k10_3d_sweep
    const char* e = getenv("TSU_POTTS_SMALL");
    return e && atoi(e) == 0;
}

bool hb_small_route(const tsu_potts3d* L) { return !small_switch_off() && sites_of(L) <= kSmallSites; }

int hb_check(tsu_potts3d* L, double T, int n_sweeps, uint32_t replica, PottsTab6* tab) {
    tsu_ctx* ctx = L->ctx;
    const char* why = potts_tables6(L->q, L->J, L->h, T, tab);
    TSU_REQUIRE(ctx, !why, "potts3d_sweep: %s", why);
    TSU_REQUIRE(ctx, n_sweeps >= 0, "potts3d_sweep: n_sweeps must be >= 0");
    TSU_REQUIRE_REPLICA(ctx, replica, "potts3d_sweep");
    return TSU_OK;
}

Potts3Geom geom_of(const tsu_potts3d* L) { return Potts3Geom{L->depth, L->rows, L->cols, L->pz, L->pr, L->pc}; }

int hb_sweep(tsu_potts3d* L, const PottsTab6& tab, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica) {
    tsu_ctx* ctx = L->ctx;
    if (n_sweeps == 0) return TSU_OK;
    Potts3Sweep p;
    p.s = L->d_s;
    p.g = geom_of(L);
    p.k = PottsKeys{(uint32_t)seed, (uint32_t)(seed >> 32), TSU_TAG_ISING_HI | (replica << 8), TSU_TAG_ISING_LO | (replica << 8)};
    p.t = tab;
    const long long lanes = (long long)L->depth * L->rows * ((L->cols + 15) >> 4);
    if (hb_small_route(L)) {
        p.hs = sweep0;
        hipLaunchKernelGGL(k10_3d_small, dim3(1), dim3((unsigned)sw_threads(lanes)), 0, ctx->stream, p, n_sweeps);
        L->launches += 1;
    } else {
        for (int k = 0; k < n_sweeps; ++k)
            for (uint32_t colour = 0; colour < 2; ++colour) {
                p.hs = 2u * (sweep0 + (uint32_t)k) + colour;  // 32-bit words: the header says so
                if ((L->cols & 15) == 0) hipLaunchKernelGGL(k10_3d_sweep<true>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, ctx->stream, p);
                else hipLaunchKernelGGL(k10_3d_sweep<false>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, ctx->stream, p);
                L->launches += 1;
            }
    }
    TSU_HIP_TRY(ctx, hipGetLastError());
    return TSU_OK;
}

int measure_into(tsu_potts3d* L, long long* d_row) {
    tsu_ctx* ctx = L->ctx;
    TSU_HIP_TRY(ctx, hipMemsetAsync(d_row, 0, TSU_POTTS_RECORD_WORDS * sizeof(long long), ctx->stream));
    Potts3Measure m = {L->d_s, geom_of(L), L->q, (unsigned long long*)d_row};
    const long long want = (sites_of(L) + 255) / 256;
    hipLaunchKernelGGL(k10_3d_measure, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(256), 0, ctx->stream, m);
    TSU_HIP_TRY(ctx, hipGetLastError());
    L->launches += 1;
    return TSU_OK;
}

}  // namespace

extern "C" {

int tsu_potts3d_check_model(int q, double J, const double* h, double T, double* tables) {
    PottsTab6 t;
    if (potts_tables6(q, J, h, T, &t)) return TSU_E_INVALID;
    if (tables) {
        for (int n = 0; n < 7; ++n) tables[n] = t.E[n];
        for (int c = 0; c < TSU_POTTS_MAX_Q; ++c) tables[7 + c] = t.F[c];
    }
    return TSU_OK;
}

int tsu_potts3d_create(tsu_ctx* ctx, int depth, int rows, int cols, int q, int pz, int pr, int pc, tsu_potts3d** out) {
    TSU_ENTER(ctx);
    if (!ctx || !out) return TSU_E_INVALID;
    TSU_REQUIRE(ctx, q >= 2 && q <= TSU_POTTS_MAX_Q, "potts3d_create: q must be in 2 .. 8 (got %d)", q);
    TSU_REQUIRE(ctx, depth >= 1 && rows >= 1 && cols >= 1, "potts3d_create: depth, rows and cols must be >= 1");
    TSU_REQUIRE(ctx, (long long)depth * rows < (1ll << 31) && (long long)depth * rows * cols < (1ll << 31),
                "potts3d_create: %lld x %d sites exceed 32-bit labels", (long long)depth * rows, cols);
    TSU_REQUIRE(ctx, (!pz || (depth & 1) == 0) && (!pr || (rows & 1) == 0) && (!pc || (cols & 1) == 0),
                "potts3d_create: a periodic axis needs an even length");
    tsu_potts3d* L = new tsu_potts3d();
    L->ctx = ctx;
    L->depth = depth;
    L->rows = rows;
    L->cols = cols;
    L->q = q;
    L->pz = pz != 0;
    L->pr = pr != 0;
    L->pc = pc != 0;
    L->J = 1.0;
    const size_t n = (size_t)depth * rows * cols;
    hipError_t e = hipMalloc((void**)&L->d_s, n);
    if (e == hipSuccess) e = hipMalloc((void**)&L->d_obs, TSU_POTTS_RECORD_WORDS * sizeof(long long));
    if (e == hipSuccess) e = hipMemsetAsync(L->d_s, 0, n, ctx->stream);
    if (e != hipSuccess) {
        if (L->d_s) (void)hipFree(L->d_s);
        if (L->d_obs) (void)hipFree(L->d_obs);
        delete L;
        return tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "potts3d_create: %s", hipGetErrorString(e));
    }
    *out = L;
    return TSU_OK;
}

int tsu_potts3d_destroy(tsu_potts3d* L) {
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

int tsu_potts3d_set_model(tsu_potts3d* L, double J, const double* h) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    TSU_REQUIRE(L->ctx, isfinite(J), "potts3d_set_model: J must be finite");
    for (int c = 0; h && c < L->q; ++c) TSU_REQUIRE(L->ctx, isfinite(h[c]), "potts3d_set_model: h must be finite");
    L->J = J;  // the bound on (6 |J| + max h - min h) / T is checked with every sweep's temperature
    for (int c = 0; c < TSU_POTTS_MAX_Q; ++c) L->h[c] = (h && c < L->q) ? h[c] : 0.0;
    return TSU_OK;
}

int tsu_potts3d_set_spins(tsu_potts3d* L, const int8_t* colours) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, colours, "potts3d_set_spins: colours is NULL");
    const size_t n = (size_t)sites_of(L);
    for (size_t i = 0; i < n; ++i)
        TSU_REQUIRE(ctx, colours[i] >= 0 && colours[i] < L->q, "potts3d_set_spins: colour %d at site %zu is outside 0 .. %d", (int)colours[i], i, L->q - 1);
    TSU_HIP_TRY(ctx, hipMemcpyAsync(L->d_s, colours, n, hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int tsu_potts3d_get_spins(tsu_potts3d* L, int8_t* colours) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, colours, "potts3d_get_spins: colours is NULL");
    TSU_HIP_TRY(ctx, hipMemcpyAsync(colours, L->d_s, (size_t)sites_of(L), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return check_err(L);
}

int tsu_potts3d_fill(tsu_potts3d* L, int colour) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    TSU_REQUIRE(L->ctx, colour >= 0 && colour < L->q, "potts3d_fill: colour %d is outside 0 .. %d", colour, L->q - 1);
    TSU_HIP_TRY(L->ctx, hipMemsetAsync(L->d_s, colour, (size_t)sites_of(L), L->ctx->stream));
    return TSU_OK;
}

int tsu_potts3d_sweep(tsu_potts3d* L, double T, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    PottsTab6 tab;
    const int rc = hb_check(L, T, n_sweeps, replica, &tab);
    if (rc != TSU_OK) return rc;
    return hb_sweep(L, tab, n_sweeps, seed, sweep0, replica);
}

int tsu_potts3d_cluster_sweep(tsu_potts3d* L, double T, int n_steps, uint64_t seed, uint32_t step0, uint32_t replica) {
    TSU_ENTER(L ? L->ctx : nullptr);
    return sw_sweep<K10x3>(L, K10x3::Model{T}, n_steps, seed, step0, replica);
}

int tsu_potts3d_route(tsu_potts3d* L, int algorithm, int* route) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L || !route) return TSU_E_INVALID;
    TSU_REQUIRE(L->ctx, algorithm == TSU_POTTS_HEAT_BATH || algorithm == TSU_POTTS_SWENDSEN_WANG, "potts3d_route: unknown algorithm %d", algorithm);
    if (algorithm == TSU_POTTS_HEAT_BATH) *route = hb_small_route(L) ? TSU_POTTS3D_ROUTE_SMALL : TSU_POTTS3D_ROUTE_SWEEP;
    else *route = sw_small_route<K10x3>(L) ? TSU_POTTS3D_ROUTE_SW_SMALL : TSU_POTTS3D_ROUTE_SW_TILES;
    return TSU_OK;
}

int tsu_potts3d_measure(tsu_potts3d* L, int64_t* row) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, row, "potts3d_measure: row is NULL");
    const int rc = measure_into(L, L->d_obs);
    if (rc != TSU_OK) return rc;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(row, L->d_obs, TSU_POTTS_RECORD_WORDS * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return check_err(L);
}

int tsu_potts3d_run(tsu_potts3d* L, double T, int n_meas, int sweeps_between, int algorithm, uint64_t seed, uint32_t counter0,
                    uint32_t replica) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, algorithm == TSU_POTTS_HEAT_BATH || algorithm == TSU_POTTS_SWENDSEN_WANG, "potts3d_run: unknown algorithm %d", algorithm);
    TSU_REQUIRE(ctx, n_meas >= 0 && sweeps_between >= 0, "potts3d_run: n_meas and sweeps_between must be >= 0");
    const long long total = (long long)n_meas * sweeps_between;
    TSU_REQUIRE(ctx, total <= (1ll << 31), "potts3d_run: %lld updates exceed one call", total);
    PottsTab6 tab;
    int rc;
    if (algorithm == TSU_POTTS_HEAT_BATH) {
        rc = hb_check(L, T, sweeps_between, replica, &tab);
    } else {
        rc = sw_check_call<K10x3>(L, K10x3::Model{T}, 0, counter0, replica);
    }
    if (rc != TSU_OK) return rc;
    TSU_REQUIRE(ctx, algorithm == TSU_POTTS_HEAT_BATH || (uint64_t)counter0 + (uint64_t)total <= (1ull << 32), "potts3d_run: step counter overflow");
    const size_t bytes = (size_t)n_meas * TSU_POTTS_RECORD_WORDS * sizeof(long long);
    TSU_HIP_TRY(ctx, ising2d_grow(L->d_rec, L->rec_cap, bytes ? bytes : sizeof(long long)));
    L->rec_rows = 0;
    for (int k = 0; k < n_meas; ++k) {
        const uint32_t c0 = counter0 + (uint32_t)((long long)k * sweeps_between);
        rc = algorithm == TSU_POTTS_HEAT_BATH ? hb_sweep(L, tab, sweeps_between, seed, c0, replica)
                                              : sw_sweep<K10x3>(L, K10x3::Model{T}, sweeps_between, seed, c0, replica);
        if (rc == TSU_OK) rc = measure_into(L, L->d_rec + (size_t)k * TSU_POTTS_RECORD_WORDS);
        if (rc != TSU_OK) return rc;
        L->rec_rows = k + 1;
    }
    return TSU_OK;
}

int tsu_potts3d_record(tsu_potts3d* L, int64_t* rows, int max_rows, int* n_rows) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, n_rows && max_rows >= 0 && (rows || max_rows == 0), "potts3d_record: n_rows is NULL, max_rows negative or rows NULL");
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const int rc = check_err(L);
    if (rc != TSU_OK) return rc;
    *n_rows = L->rec_rows;
    const int n = L->rec_rows < max_rows ? L->rec_rows : max_rows;
    if (n > 0) TSU_HIP_TRY(ctx, hipMemcpy(rows, L->d_rec, (size_t)n * TSU_POTTS_RECORD_WORDS * sizeof(int64_t), hipMemcpyDeviceToHost));
    return TSU_OK;
}

int tsu_potts3d_launch_count(tsu_potts3d* L, uint64_t* n) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L || !n) return TSU_E_INVALID;
    *n = L->launches + L->sw.launches;
    return TSU_OK;
}

}  // extern "C"

// ising3d_cluster.hip -- K8: Swendsen-Wang cluster steps on the 3-D lattice handle, per-bond couplings of either sign (gfx950).
//
// One step at zero field: bonds -> connected components -> one coin per component.  Step t of a D x R x C lattice, key = seed,
// global row rho = z R + r, site index i = rho C + c (the bit-exact contract):
//   bond    b = (i, j) with stored fp32 coupling J_b is active iff J_b s_i s_j > 0 and u_b < thr_b,
//           thr_b = floor(p_b 2^32), p_b = -expm1(-2 |J_b| / T) in float64 from the fp32 value widened (thr_b may be 2^32: a
//           64-bit compare).  J_b = 0 is never active, so the zero last slices of an open axis need no special case; the
//           neighbour across an open edge is still not read.
//   u_b     right and down bonds of (z, r, c): K6's words with rho in place of r, W = Philox(c >> 1, rho, t, TAG_SW_BOND | rep << 8),
//           right W[2 (c & 1)], down W[2 (c & 1) + 1]; the layer bond to (z + 1, r, c) (to z = 0 across a periodic z axis): word
//           c & 3 of Philox(c >> 2, rho, t, TAG_SW_LAYER | rep << 8)
//   labels  union-find with min-index roots (uf_dev.h): the root of a finished tree is its component's smallest site index
//   flip    the cluster rooted at (rho, c) flips iff flip_bit(rho, c, t, TAG_SW_FLIP | rep << 8, key)
// With D = 1, open z and constant J this is tsu_ising2d_cluster_sweep on R x C bit for bit.
// Two routes, the same counters and hence the same spins:
//   k8_sw_small    a whole lattice of at most 16384 sites in one workgroup's LDS (4 B labels + 1 B spins a site, 80 KB at most)
//                  for all steps of a call; workgroup b of a launch runs lattice b of a batch with its own disorder pointers.
//                  The bond thresholds are recomputed every step from J in L2 (no LDS for them: caching 3 x 8 B a site would
//                  not fit beside the labels)
//   k8_sw_local    one workgroup per tz x tr x tc tile: the tile's inner bonds and union-find in LDS, tile-root labels to HBM
//   k8_sw_merge    one lane per bond across a tile face or a wrap, all three axes: the bond recomputed from the spins, the
//                  coupling and the same Philox word, the two roots joined in HBM (agent-scope atomicMin)
//   k8_sw_resolve  one lane per 4 sites: label -> root, the root's coin, the spin rewritten in place (pad bytes stay 0)
// Nothing waits on another workgroup.  Every union / find loop draws on a per-lane budget; when it runs out the kernel raises
// h_err = 2 and gives up on that bond instead of spinning (the next synchronising call of the handle reports it); on the small
// route the lattice then keeps the spins it had before the call.
// In a field (tsu_ising3d_cluster_sweep_field, the <true> instantiations of the four kernels): every site has one more bond, to a
// ghost spin fixed at +1:
//   ghost   the bond of site i with stored fp32 field h_i is active iff h_i s_i > 0 and u_g < thr(|h_i|) (the same thr, 64-bit
//           compare; h_i = 0 is never active), u_g = word c & 3 of Philox(c >> 2, rho, t, TAG_SW_GHOST | rep << 8)
//   frozen  a component with an active ghost bond keeps its spins and draws no coin; every other one flips by its root's coin
// The ghost is label -1 (uf_dev.h, ufg_find / ufg_union): an index below every site, so the min-index union-find takes it as it
// is.  k8_sw_local writes -1 as the global label of a site whose tile root is frozen, k8_sw_merge takes -1 on either side,
// k8_sw_resolve reads a negative root as "no flip".  No extra array, LDS or launch; with h = 0 everywhere the spins are those of
// the zero-field step.  The <false> instantiations are the zero-field kernels as they were.
// No fp32 screen of u_b: only satisfied bonds (J s s' > 0) reach the float64 expm1, and the kernels are bound by the LDS / L2
// atomics of the union-find, not by it.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ising2d.h"
#include "ising3d.h"
#include "uf_dev.h"

namespace {

constexpr int kSmallSites = 16384;  // k8_sw_small: depth * rows * cols at most this (80 KB of LDS); also the largest tile
constexpr int kMaxThreads = 1024;

// J s s' > 0 and u < thr(J, T)
__device__ __forceinline__ bool bond3_on(float J, int sa, int sb, uint32_t u, double T) {
    const int js = (J > 0.0f) - (J < 0.0f);
    if (js * sa * sb <= 0) return false;
    const double p = -expm1((-2.0 * fabs((double)J)) / T);
    return (uint64_t)u < (uint64_t)floor(p * 4294967296.0);
}

// h s > 0: the ghost bond of the site can be active (bond3_on(h, s, 1, u_g, T) then decides)
__device__ __forceinline__ bool ghost_sat(float h, int s) { return ((h > 0.0f) - (h < 0.0f)) * s > 0; }

__device__ __forceinline__ uint32_t word_of(const u32x4& w, int m) { return m == 0 ? w.x : (m == 1 ? w.y : (m == 2 ? w.z : w.w)); }

// ---------------------------------------------------------------- one workgroup per lattice
struct Sw3Item {
    int8_t* s;
    const float* jr;
    const float* jd;
    const float* jl;
    const float* h;  // read by the ghost kernels only
    double T;
    uint32_t k0, k1, tag_bond, tag_layer, tag_flip, tag_ghost, step0;
};

// the union / find of a kernel: with a ghost, label -1 is legal
template <bool GHOST, int SCOPE>
__device__ __forceinline__ bool sw_union(int* L, int a, int b, int& budget) {
    if constexpr (GHOST) return ufg_union<SCOPE>(L, a, b, budget);
    else return uf_union<SCOPE>(L, a, b, budget);
}

template <bool GHOST, int SCOPE>
__device__ __forceinline__ int sw_find(int* L, int x, int& budget) {
    if constexpr (GHOST) return ufg_find<SCOPE>(L, x, budget);
    else return uf_find<SCOPE>(L, x, budget);
}

template <bool GHOST>
__global__ __launch_bounds__(kMaxThreads) void k8_sw_small(const Sw3Item* __restrict__ items, Sw3Item one, int depth, int rows, int cols,
                                                           long long pitch, int pz, int pr, int pc, int n_steps, int* err) {
    extern __shared__ int s_lab[];
    __shared__ int s_bad;
    const Sw3Item& it = items ? items[blockIdx.x] : one;
    const int nrows = depth * rows, n = nrows * cols, tid = threadIdx.x, nt = blockDim.x;
    int8_t* const s_spin = reinterpret_cast<int8_t*>(s_lab + n);
    if (tid == 0) s_bad = 0;
    for (int i = tid; i < n; i += nt) {
        const int rho = i / cols, c = i - rho * cols;
        s_spin[i] = it.s[(long long)rho * pitch + c];
    }
    const int hc = (cols + 1) >> 1, npairs = nrows * hc;
    for (int s = 0; s < n_steps; ++s) {
        const uint32_t t = it.step0 + (uint32_t)s;
        for (int i = tid; i < n; i += nt) s_lab[i] = i;
        __syncthreads();
        int budget = kBudget;
        for (int p = tid; p < npairs; p += nt) {
            const int rho = p / hc, cp = p - rho * hc;
            const int z = rho / rows, r = rho - z * rows;
            const u32x4 w = tsu_philox((uint32_t)cp, (uint32_t)rho, t, it.tag_bond, it.k0, it.k1);
            const u32x4 wl = tsu_philox((uint32_t)cp >> 1, (uint32_t)rho, t, it.tag_layer, it.k0, it.k1);
            const int rd = r + 1 < rows ? rho + 1 : (pr ? z * rows : -1);      // global row of the down neighbour
            const int rf = z + 1 < depth ? rho + rows : (pz ? r : -1);         // ... of the layer neighbour
            u32x4 wg = {0u, 0u, 0u, 0u};  // the ghost bonds' block, drawn once a site of the pair has h s > 0
            bool have_wg = false;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = 2 * cp + j;
                if (c >= cols) break;
                const int i = rho * cols + c, si = s_spin[i];
                const long long g = (long long)rho * pitch + c;
                const int cr = c + 1 < cols ? c + 1 : (pc ? 0 : -1);
                const float h = GHOST ? it.h[g] : 0.0f;  // read ahead of the unions, whose atomics it would otherwise wait behind
                if (cr >= 0 && bond3_on(it.jr[g], si, s_spin[rho * cols + cr], j ? w.z : w.x, it.T))
                    if (!sw_union<GHOST, __HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, i, rho * cols + cr, budget)) s_bad = 1;
                if (rd >= 0 && bond3_on(it.jd[g], si, s_spin[rd * cols + c], j ? w.w : w.y, it.T))
                    if (!sw_union<GHOST, __HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, i, rd * cols + c, budget)) s_bad = 1;
                if (rf >= 0 && bond3_on(it.jl[g], si, s_spin[rf * cols + c], word_of(wl, c & 3), it.T))
                    if (!sw_union<GHOST, __HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, i, rf * cols + c, budget)) s_bad = 1;
                if constexpr (GHOST) {
                    if (ghost_sat(h, si)) {
                        if (!have_wg) wg = tsu_philox((uint32_t)cp >> 1, (uint32_t)rho, t, it.tag_ghost, it.k0, it.k1);
                        have_wg = true;
                        if (bond3_on(h, si, 1, word_of(wg, c & 3), it.T))
                            if (!ufg_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, i, -1, budget)) s_bad = 1;
                    }
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < n; i += nt) {
            budget = kBudget;
            const int root = sw_find<GHOST, __HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, i, budget);
            if (budget < 0) s_bad = 1;
            if (GHOST && root < 0) continue;  // frozen: no coin
            const int rr = root / cols, rc = root - rr * cols;
            if (flip_bit(rr, rc, t, it.tag_flip, it.k0, it.k1)) s_spin[i] = (int8_t)-s_spin[i];
        }
        __syncthreads();
        if (s_bad) break;
    }
    if (s_bad) {
        if (tid == 0) raise_err(err);
        return;  // the lattice keeps its spins from before the call
    }
    for (int i = tid; i < n; i += nt) {
        const int rho = i / cols, c = i - rho * cols;
        it.s[(long long)rho * pitch + c] = s_spin[i];
    }
}

// ---------------------------------------------------------------- multi-tile route
struct Sw3Params {
    int8_t* s;
    const float* jr;
    const float* jd;
    const float* jl;
    const float* h;  // read by the ghost kernels only
    int* labels;  // depth * rows * cols; -1 (ghost kernels only): the site's component is frozen
    long long pitch;
    int depth, rows, cols;
    int pz, pr, pc;
    int tz, tr, tc;  // tile shape (tc even: a right / down Philox block never straddles two tiles)
    int nz, nr, nc;  // tiles per axis
    double T;
    uint32_t k0, k1, tag_bond, tag_layer, tag_flip, tag_ghost, t;
    int* err;
};

// tile blockIdx.x (row-major over nz x nr x nc) of tz x tr x tc sites; bonds with both ends in the tile, none across its faces
// or a wrap.  LDS: tz*tr*tc int32 labels (tile-local, row-major: the same order as the global indices inside a tile) and as many
// spins.  Writes the global index of every site's tile root; GHOST: the ghost bond of every site of the tile too, and -1 where the
// tile root is frozen.
template <bool GHOST>
__global__ __launch_bounds__(kMaxThreads) void k8_sw_local(Sw3Params p) {
    extern __shared__ int s_lab[];
    const int TZ = p.tz, TR = p.tr, TC = p.tc, n = TZ * TR * TC;
    int8_t* const s_spin = reinterpret_cast<int8_t*>(s_lab + n);
    const int bz = (int)(blockIdx.x / (unsigned)(p.nr * p.nc)), brc = (int)blockIdx.x - bz * p.nr * p.nc;
    const int br = brc / p.nc, bc = brc - br * p.nc;
    const int z0 = bz * TZ, r0 = br * TR, c0 = bc * TC;
    const int tz = p.depth - z0 < TZ ? p.depth - z0 : TZ, tr = p.rows - r0 < TR ? p.rows - r0 : TR, tc = p.cols - c0 < TC ? p.cols - c0 : TC;
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int i = tid; i < n; i += nt) {
        const int lz = i / (TR * TC), rem = i - lz * TR * TC, lr = rem / TC, lc = rem - lr * TC;
        s_lab[i] = i;
        s_spin[i] = (lz < tz && lr < tr && lc < tc) ? p.s[((long long)(z0 + lz) * p.rows + r0 + lr) * p.pitch + c0 + lc] : (int8_t)0;
    }
    __syncthreads();
    int budget = kBudget;
    bool bad = false;
    const int hw = TC >> 1;
    for (int q = tid; q < TZ * TR * hw; q += nt) {
        const int lz = q / (TR * hw), rem = q - lz * TR * hw, lr = rem / hw, lc0 = 2 * (rem - lr * hw);
        if (lz >= tz || lr >= tr || lc0 >= tc) continue;
        const long long rho = (long long)(z0 + lz) * p.rows + r0 + lr;
        const u32x4 w = tsu_philox((uint32_t)(c0 + lc0) >> 1, (uint32_t)rho, p.t, p.tag_bond, p.k0, p.k1);
        const u32x4 wl = tsu_philox((uint32_t)(c0 + lc0) >> 2, (uint32_t)rho, p.t, p.tag_layer, p.k0, p.k1);
        u32x4 wg = {0u, 0u, 0u, 0u};
        bool have_wg = false;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int lc = lc0 + j;
            if (lc >= tc) break;
            const int i = (lz * TR + lr) * TC + lc, si = s_spin[i];
            const long long g = rho * p.pitch + c0 + lc;
            const float h = GHOST ? p.h[g] : 0.0f;  // read ahead of the unions, whose atomics it would otherwise wait behind
            if (lc + 1 < tc && bond3_on(p.jr[g], si, s_spin[i + 1], j ? w.z : w.x, p.T))
                bad |= !sw_union<GHOST, __HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, i, i + 1, budget);
            if (lr + 1 < tr && bond3_on(p.jd[g], si, s_spin[i + TC], j ? w.w : w.y, p.T))
                bad |= !sw_union<GHOST, __HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, i, i + TC, budget);
            if (lz + 1 < tz && bond3_on(p.jl[g], si, s_spin[i + TR * TC], word_of(wl, (c0 + lc) & 3), p.T))
                bad |= !sw_union<GHOST, __HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, i, i + TR * TC, budget);
            if constexpr (GHOST) {
                if (ghost_sat(h, si)) {
                    if (!have_wg) wg = tsu_philox((uint32_t)(c0 + lc0) >> 2, (uint32_t)rho, p.t, p.tag_ghost, p.k0, p.k1);
                    have_wg = true;
                    if (bond3_on(h, si, 1, word_of(wg, (c0 + lc) & 3), p.T))
                        bad |= !ufg_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, i, -1, budget);
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += nt) {
        const int lz = i / (TR * TC), rem = i - lz * TR * TC, lr = rem / TC, lc = rem - lr * TC;
        if (lz >= tz || lr >= tr || lc >= tc) continue;
        budget = kBudget;
        const int root = sw_find<GHOST, __HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, i, budget);
        bad |= budget < 0;
        const int rz = root / (TR * TC), rrem = root - rz * TR * TC, rr = rrem / TC, rc = rrem - rr * TC;
        const int label = ((z0 + rz) * p.rows + r0 + rr) * p.cols + c0 + rc;
        p.labels[((long long)(z0 + lz) * p.rows + r0 + lr) * p.cols + c0 + lc] = (GHOST && root < 0) ? -1 : label;
    }
    if (bad) raise_err(p.err);
}

// lanes [0, sc D R): right bonds of the column seams (seam k < nc - 1 at column (k + 1) tc - 1, the last one of a periodic axis at
// column cols - 1, wrapping to 0); then sr D C lanes for the down bonds of the row seams; then sz R C lanes for the layer bonds.
// GHOST: either label may be -1 (a frozen tile root); joining it with a free root freezes that root's tree
template <bool GHOST>
__global__ __launch_bounds__(256) void k8_sw_merge(Sw3Params p, int sc, int sr, int sz) {
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long nrows = (long long)p.depth * p.rows;
    const long long lc_n = (long long)sc * nrows, lr_n = (long long)sr * p.depth * p.cols, lz_n = (long long)sz * p.rows * p.cols;
    if (lane >= lc_n + lr_n + lz_n) return;
    long long rho, rho2;
    int c, c2, axis;
    if (lane < lc_n) {
        const int k = (int)(lane / nrows);
        rho = rho2 = lane - (long long)k * nrows;
        c = k < p.nc - 1 ? (k + 1) * p.tc - 1 : p.cols - 1;
        c2 = c + 1 < p.cols ? c + 1 : 0;
        axis = 0;
    } else if (lane < lc_n + lr_n) {
        const long long l = lane - lc_n, per = (long long)p.depth * p.cols;
        const int k = (int)(l / per);
        const long long rem = l - (long long)k * per;
        const int z = (int)(rem / p.cols);
        c = c2 = (int)(rem - (long long)z * p.cols);
        const int r = k < p.nr - 1 ? (k + 1) * p.tr - 1 : p.rows - 1;
        rho = (long long)z * p.rows + r;
        rho2 = (long long)z * p.rows + (r + 1 < p.rows ? r + 1 : 0);
        axis = 1;
    } else {
        const long long l = lane - lc_n - lr_n, per = (long long)p.rows * p.cols;
        const int k = (int)(l / per);
        const long long rem = l - (long long)k * per;
        const int r = (int)(rem / p.cols);
        c = c2 = (int)(rem - (long long)r * p.cols);
        const int z = k < p.nz - 1 ? (k + 1) * p.tz - 1 : p.depth - 1;
        rho = (long long)z * p.rows + r;
        rho2 = (long long)(z + 1 < p.depth ? z + 1 : 0) * p.rows + r;
        axis = 2;
    }
    const int sa = p.s[rho * p.pitch + c], sb = p.s[rho2 * p.pitch + c2];
    const float J = (axis == 0 ? p.jr : (axis == 1 ? p.jd : p.jl))[rho * p.pitch + c];
    const int js = (J > 0.0f) - (J < 0.0f);
    if (js * sa * sb <= 0) return;
    uint32_t u;
    if (axis == 2) {
        u = word_of(tsu_philox((uint32_t)c >> 2, (uint32_t)rho, p.t, p.tag_layer, p.k0, p.k1), c & 3);
    } else {
        u = word_of(tsu_philox((uint32_t)c >> 1, (uint32_t)rho, p.t, p.tag_bond, p.k0, p.k1), 2 * (c & 1) + axis);
    }
    if (!bond3_on(J, sa, sb, u, p.T)) return;
    int budget = kBudget;
    const int a = p.labels[rho * p.cols + c], b = p.labels[rho2 * p.cols + c2];
    if (!sw_union<GHOST, __HIP_MEMORY_SCOPE_AGENT>(p.labels, a, b, budget)) raise_err(p.err);
}

// one lane per 4 sites of a global row (one 4-byte load and store; the pad bytes beyond cols are 0 and stay 0): the root of each
// site, the root's coin (one Philox block per distinct root of the lane), the spin rewritten.  GHOST: a chain that ends in -1 is a
// frozen component: no coin, the spin stays
template <bool GHOST>
__global__ __launch_bounds__(256) void k8_sw_resolve(Sw3Params p, int quads) {
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long rho = lane / quads;
    const int c0 = 4 * (int)(lane - rho * quads);
    if (rho >= (long long)p.depth * p.rows) return;
    int8_t* const row = p.s + rho * p.pitch;
    uint32_t v = *reinterpret_cast<const uint32_t*>(row + c0);
    int last = -1;
    bool last_flip = false, bad = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (c0 + j >= p.cols) break;
        const long long g = rho * p.cols + c0 + j;
        int x = p.labels[g], budget = kBudget;
        if (!GHOST || x >= 0) {
            for (int y = p.labels[x]; y != x; y = p.labels[x]) {
                x = y;
                if (GHOST && x < 0) break;
                if (--budget < 0) {
                    bad = true;
                    break;
                }
            }
        }
        if (GHOST && x < 0) {
            last = x;
            last_flip = false;
        } else if (x != last) {
            const int rr = x / p.cols, rc = x - rr * p.cols;
            last = x;
            last_flip = flip_bit(rr, rc, p.t, p.tag_flip, p.k0, p.k1);
        }
        if (last_flip) {
            const uint32_t b = (v >> (8 * j)) & 0xFFu;
            v = (v & ~(0xFFu << (8 * j))) | (((uint32_t)(-(int)(int8_t)b) & 0xFFu) << (8 * j));
        }
    }
    *reinterpret_cast<uint32_t*>(row + c0) = v;
    if (bad) raise_err(p.err);
}

// ---------------------------------------------------------------- host side
struct Tile {
    int z, r, c;
};

// TSU_SW3D_TILE=<tz>x<tr>x<tc> (tests only, read per call): that tile shape, and every lattice on the multi-tile route.
// 1: a shape was read; 0: the switch is not set; -1: it does not parse
int tile_switch(Tile* t) {
    const char* e = getenv("TSU_SW3D_TILE");
    if (!e || !*e) return 0;
    char tail = 0;
    return sscanf(e, "%dx%dx%d%c", &t->z, &t->r, &t->c, &tail) == 3 ? 1 : -1;
}

long long sites_of(const tsu_ising3d* L) { return (long long)L->depth * L->rows * L->cols; }

bool small_route(const tsu_ising3d* L) {
    Tile t;
    return tile_switch(&t) == 0 && sites_of(L) <= kSmallSites;
}

// The default tile.  16 x 32 x 32 (80 KB of LDS, 1024 lanes, two tiles a CU) leaves 1/16 + 1/32 + 1/32 = 12.5 % of a site's
// three bonds' worth on seams (4.2 % of the bonds); 8 x 16 x 32 (20 KB, 256 lanes) leaves 21.9 % (7.3 % of the bonds) but gives four
// times the workgroups.  The large tile is taken once it fills the chip (one tile per CU at least), the small one below that
// (DESIGN.md section 5, K8 cluster steps).
Tile default_tile(const tsu_ising3d* L) {
    const Tile big = {16, 32, 32}, small = {8, 16, 32};
    const long long n_big = (long long)((L->depth + big.z - 1) / big.z) * ((L->rows + big.r - 1) / big.r) * ((L->cols + big.c - 1) / big.c);
    return n_big >= (L->ctx->cus > 0 ? L->ctx->cus : 256) ? big : small;
}

int ensure_err(tsu_ising3d* L, int** d_err) {
    tsu_ctx* ctx = L->ctx;
    if (!L->h_err) {
        TSU_HIP_TRY(ctx, hipHostMalloc(&L->h_err, sizeof(int), hipHostMallocMapped));
        *L->h_err = 0;
    }
    TSU_HIP_TRY(ctx, hipHostGetDevicePointer((void**)d_err, L->h_err, 0));
    return TSU_OK;
}

Sw3Item make_item(const tsu_ising3d* L, double T, uint64_t seed, uint32_t step0, uint32_t replica) {
    const size_t plane = (size_t)L->depth * L->rows * L->pitch;
    Sw3Item it;
    it.s = L->s;
    it.jr = L->d_dis;
    it.jd = L->d_dis + plane;
    it.jl = L->d_dis + 2 * plane;
    it.h = L->d_dis + 3 * plane;  // zeros when no field was given
    it.T = T;
    it.k0 = (uint32_t)seed;
    it.k1 = (uint32_t)(seed >> 32);
    it.tag_bond = TSU_TAG_SW_BOND | (replica << 8);
    it.tag_layer = TSU_TAG_SW_LAYER | (replica << 8);
    it.tag_flip = TSU_TAG_SW_FLIP | (replica << 8);
    it.tag_ghost = TSU_TAG_SW_GHOST | (replica << 8);
    it.step0 = step0;
    return it;
}

int threads_for(long long work_items) {
    const long long t = (work_items + 63) / 64 * 64;
    return (int)(t < kMaxThreads ? t : kMaxThreads);
}

template <bool GHOST>
int run_small(tsu_ising3d* const* lats, int n, const Sw3Item* items, int n_steps) {
    tsu_ising3d* L0 = lats[0];
    tsu_ctx* ctx = L0->ctx;
    int* d_err = nullptr;
    int rc = ensure_err(L0, &d_err);
    if (rc != TSU_OK) return rc;
    const size_t lds = (size_t)sites_of(L0) * 5;
    TSU_HIP_TRY(ctx, tsu_func_allow_lds(ctx, (const void*)k8_sw_small<GHOST>, (int)lds));
    const Sw3Item* d_items = nullptr;
    if (n > 1) {
        const size_t bytes = (size_t)n * sizeof(Sw3Item);
        TSU_HIP_TRY(ctx, ising2d_grow(L0->d_sw_batch, L0->sw_batch_cap, bytes));
        // the host array dies with this call: wait for the copy (a few KB); the launch itself stays asynchronous
        TSU_HIP_TRY(ctx, hipMemcpyAsync(L0->d_sw_batch, items, bytes, hipMemcpyHostToDevice, ctx->stream));
        TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        d_items = (const Sw3Item*)L0->d_sw_batch;
    }
    const int threads = threads_for((long long)L0->depth * L0->rows * ((L0->cols + 1) / 2));
    hipLaunchKernelGGL(k8_sw_small<GHOST>, dim3((unsigned)n), dim3((unsigned)threads), lds, ctx->stream, d_items, items[0], L0->depth, L0->rows,
                       L0->cols, (long long)L0->pitch, L0->pz, L0->pr, L0->pc, n_steps, d_err);
    TSU_HIP_TRY(ctx, hipGetLastError());
    for (int i = 0; i < n; ++i) lats[i]->sw_launches += 1;
    return TSU_OK;
}

template <bool GHOST>
int run_tiles(tsu_ising3d* L, const Sw3Item& it, int n_steps) {
    tsu_ctx* ctx = L->ctx;
    Tile t;
    const int sw = tile_switch(&t);
    TSU_REQUIRE(ctx, sw >= 0, "TSU_SW3D_TILE must read <tz>x<tr>x<tc>");
    if (sw == 0) t = default_tile(L);
    TSU_REQUIRE(ctx, t.z >= 1 && t.r >= 1 && t.c >= 2 && (t.c & 1) == 0 && t.z <= kSmallSites && t.r <= kSmallSites && t.c <= kSmallSites &&
                         (long long)t.z * t.r * t.c <= kSmallSites,
                "TSU_SW3D_TILE: a tile needs positive extents, an even width and at most %d sites (got %d x %d x %d)", kSmallSites, t.z, t.r, t.c);
    const size_t sites = (size_t)sites_of(L);
    {
        const hipError_t e = ising2d_grow(L->d_labels, L->labels_cap, sites * sizeof(int32_t));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "ising3d_cluster: the labels buffer: %s (%zu bytes)",
                            hipGetErrorString(e), sites * sizeof(int32_t));
        }
    }
    Sw3Params p;
    p.s = it.s;
    p.jr = it.jr;
    p.jd = it.jd;
    p.jl = it.jl;
    p.h = it.h;
    p.labels = L->d_labels;
    p.pitch = (long long)L->pitch;
    p.depth = L->depth;
    p.rows = L->rows;
    p.cols = L->cols;
    p.pz = L->pz;
    p.pr = L->pr;
    p.pc = L->pc;
    p.tz = t.z;
    p.tr = t.r;
    p.tc = t.c;
    p.nz = (L->depth + t.z - 1) / t.z;
    p.nr = (L->rows + t.r - 1) / t.r;
    p.nc = (L->cols + t.c - 1) / t.c;
    p.T = it.T;
    p.k0 = it.k0;
    p.k1 = it.k1;
    p.tag_bond = it.tag_bond;
    p.tag_layer = it.tag_layer;
    p.tag_flip = it.tag_flip;
    p.tag_ghost = it.tag_ghost;
    p.t = 0;
    int rc = ensure_err(L, &p.err);
    if (rc != TSU_OK) return rc;
    const long long n_tiles = (long long)p.nz * p.nr * p.nc;
    TSU_REQUIRE(ctx, n_tiles < (1ll << 31), "ising3d_cluster: %lld tiles exceed the grid", n_tiles);
    const int sc = p.nc - 1 + L->pc, sr = p.nr - 1 + L->pr, sz = p.nz - 1 + L->pz;
    const long long merge_lanes = (long long)sc * L->depth * L->rows + (long long)sr * L->depth * L->cols + (long long)sz * L->rows * L->cols;
    const int tile_sites = t.z * t.r * t.c;
    const size_t lds = (size_t)tile_sites * 5;
    TSU_HIP_TRY(ctx, tsu_func_allow_lds(ctx, (const void*)k8_sw_local<GHOST>, (int)lds));
    const int local_threads = threads_for((tile_sites + 15) / 16);
    const int quads = (L->cols + 3) / 4;
    const unsigned resolve_blocks = (unsigned)(((long long)quads * L->depth * L->rows + 255) / 256);
    for (int s = 0; s < n_steps; ++s) {
        p.t = it.step0 + (uint32_t)s;
        hipLaunchKernelGGL(k8_sw_local<GHOST>, dim3((unsigned)n_tiles), dim3((unsigned)local_threads), lds, ctx->stream, p);
        if (merge_lanes > 0)
            hipLaunchKernelGGL(k8_sw_merge<GHOST>, dim3((unsigned)((merge_lanes + 255) / 256)), dim3(256), 0, ctx->stream, p, sc, sr, sz);
        hipLaunchKernelGGL(k8_sw_resolve<GHOST>, dim3(resolve_blocks), dim3(256), 0, ctx->stream, p, quads);
        L->sw_launches += merge_lanes > 0 ? 3 : 2;
    }
    TSU_HIP_TRY(ctx, hipGetLastError());
    return TSU_OK;
}

int check_call(tsu_ising3d* L, double T, int n_steps, uint32_t step0, uint32_t replica, bool ghost) {
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, L->have_disorder, "ising3d_cluster_sweep: call tsu_ising3d_set_disorder first");
    TSU_REQUIRE(ctx, T > 0.0 && isfinite(T), "Temperature must be positive");
    if (L->have_field && !ghost)
        return tsu_fail(ctx, TSU_E_UNSUPPORTED, "ising3d_cluster: Swendsen-Wang cluster steps need zero field (a field would need a ghost spin)");
    if (sites_of(L) >= (1ll << 31))
        return tsu_fail(ctx, TSU_E_UNSUPPORTED, "ising3d_cluster: %lld sites exceed 32-bit labels", sites_of(L));
    TSU_REQUIRE(ctx, n_steps >= 0, "ising3d_cluster: n_steps must be >= 0");
    TSU_REQUIRE(ctx, (uint64_t)step0 + (uint64_t)n_steps <= (1ull << 32), "ising3d_cluster: step counter overflow");
    TSU_REQUIRE_REPLICA(ctx, replica, "ising3d_cluster");
    return ising3d_check_err(L);  // a cap that expired in an earlier call
}

// GHOST = false: the zero-field entry points (a stored field is refused); true: the ghost-spin ones
template <bool GHOST>
int sweep_one(tsu_ising3d* L, double T, int n_steps, uint64_t seed, uint32_t step0, uint32_t replica) {
    if (!L) return TSU_E_INVALID;
    int rc = check_call(L, T, n_steps, step0, replica, GHOST);
    if (rc != TSU_OK || n_steps == 0) return rc;
    const Sw3Item it = make_item(L, T, seed, step0, replica);
    return small_route(L) ? run_small<GHOST>(&L, 1, &it, n_steps) : run_tiles<GHOST>(L, it, n_steps);
}

template <bool GHOST>
int sweep_batch(tsu_ising3d* const* lats, int n_lats, int n_steps, const double* Ts, const uint64_t* seeds, const uint32_t* step0s,
                const uint32_t* replicas) {
    if (!lats || n_lats < 1 || !lats[0]) return TSU_E_INVALID;
    tsu_ctx* ctx = lats[0]->ctx;
    TSU_REQUIRE(ctx, Ts && seeds && step0s && replicas, "ising3d_cluster_sweep_batch: Ts, seeds, step0s and replicas are per-lattice arrays");
    const tsu_ising3d* A = lats[0];
    bool one_launch = true;  // every lattice on k8_sw_small, all of one shape and boundary
    for (int i = 0; i < n_lats; ++i) {
        tsu_ising3d* L = lats[i];
        TSU_REQUIRE(ctx, L && L->ctx == ctx, "ising3d_cluster_sweep_batch: lattice %d is NULL or belongs to another context", i);
        for (int k = 0; k < i; ++k)
            TSU_REQUIRE(ctx, lats[k] != L, "ising3d_cluster_sweep_batch: lattice %d appears twice", i);
        int rc = check_call(L, Ts[i], n_steps, step0s[i], replicas[i], GHOST);
        if (rc != TSU_OK) return rc;
        one_launch = one_launch && small_route(L) && L->depth == A->depth && L->rows == A->rows && L->cols == A->cols && L->pz == A->pz &&
                     L->pr == A->pr && L->pc == A->pc;
    }
    if (n_steps == 0) return TSU_OK;
    if (one_launch) {
        std::vector<Sw3Item> items((size_t)n_lats);
        for (int i = 0; i < n_lats; ++i) items[(size_t)i] = make_item(lats[i], Ts[i], seeds[i], step0s[i], replicas[i]);
        return run_small<GHOST>(lats, n_lats, items.data(), n_steps);
    }
    for (int i = 0; i < n_lats; ++i) {
        int rc = sweep_one<GHOST>(lats[i], Ts[i], n_steps, seeds[i], step0s[i], replicas[i]);
        if (rc != TSU_OK) return rc;
    }
    return TSU_OK;
}

}  // namespace

int ising3d_check_err(tsu_ising3d* L) {
    if (L->h_err && *L->h_err) {
        *L->h_err = 0;
        return tsu_fail(L->ctx, TSU_E_HIP, "ising3d: a cluster kernel's union / find loop hit its iteration cap; results invalid");
    }
    return TSU_OK;
}

void ising3d_cluster_free(tsu_ising3d* L) {
    if (L->d_labels) (void)hipFree(L->d_labels);
    if (L->d_sw_batch) (void)hipFree(L->d_sw_batch);
    if (L->h_err) (void)hipHostFree(L->h_err);
    L->d_labels = nullptr;
    L->d_sw_batch = nullptr;
    L->h_err = nullptr;
    L->labels_cap = L->sw_batch_cap = 0;
}

extern "C" {

int tsu_ising3d_cluster_sweep(tsu_ising3d* L, double T, int n_steps, uint64_t seed, uint32_t step0, uint32_t replica) {
    TSU_ENTER(L ? L->ctx : nullptr);
    return sweep_one<false>(L, T, n_steps, seed, step0, replica);
}

int tsu_ising3d_cluster_sweep_batch(tsu_ising3d* const* lats, int n_lats, int n_steps, const double* Ts, const uint64_t* seeds,
                                    const uint32_t* step0s, const uint32_t* replicas) {
    TSU_ENTER((lats && n_lats > 0 && lats[0]) ? lats[0]->ctx : nullptr);
    return sweep_batch<false>(lats, n_lats, n_steps, Ts, seeds, step0s, replicas);
}

int tsu_ising3d_cluster_sweep_field(tsu_ising3d* L, double T, int n_steps, uint64_t seed, uint32_t step0, uint32_t replica) {
    TSU_ENTER(L ? L->ctx : nullptr);
    return sweep_one<true>(L, T, n_steps, seed, step0, replica);
}

int tsu_ising3d_cluster_sweep_field_batch(tsu_ising3d* const* lats, int n_lats, int n_steps, const double* Ts, const uint64_t* seeds,
                                          const uint32_t* step0s, const uint32_t* replicas) {
    TSU_ENTER((lats && n_lats > 0 && lats[0]) ? lats[0]->ctx : nullptr);
    return sweep_batch<true>(lats, n_lats, n_steps, Ts, seeds, step0s, replicas);
}

int tsu_ising3d_cluster_launch_count(tsu_ising3d* L, uint64_t* n) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L || !n) return TSU_E_INVALID;
    *n = L->sw_launches;
    return TSU_OK;
}

}  // extern "C"

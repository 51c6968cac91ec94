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
// The ghost is label -1 (uf_dev.h, uf_find / uf_union with GHOST): an index below every site, so the min-index union-find takes it
// as it is.  k8_sw_local writes -1 as the global label of a site whose tile root is frozen, k8_sw_merge takes -1 on either side,
// k8_sw_resolve reads a negative root as "no flip".  No extra array, LDS or launch; with h = 0 everywhere the spins are those of
// the zero-field step.  The <false> instantiations compile every test for the ghost out.
// No fp32 screen of u_b: only satisfied bonds (J s s' > 0) reach the float64 expm1, and the kernels are bound by the LDS / L2
// atomics of the union-find, not by it.
// Shared with K6 (ising2d_cluster.hip): the structs, the bond policies, the seam decoder, the root chase and the resolve pass
// (sw_dev.h, DIM = 3) and the whole host side (sw_host.h, with the traits below).  This file keeps what only K8 has: the disorder and
// field checks, the refusal of a lattice listed twice in a batch, the labels out-of-memory
// message, the entry points, and the bodies of the kernels that run a union-find (k8_sw_small, k8_sw_local, k8_sw_merge: sw_dev.h
// says why).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "ising3d.h"
#include "sw_host.h"

namespace {

using Item = SwItem<SwStoredBonds>;
using Params = SwParams<SwStoredBonds>;

// Rec: nothing (k8_sw_small<GHOST>: the plain kernel, its arguments and code as they always were) or one SwRecOut (the measured
// instantiation of tsu_hip_cluster_measure.h: one more dword of LDS a site for the roots' counts, a row per step)
template <bool GHOST, class... Rec>
__global__ __launch_bounds__(kSwMaxThreads) void k8_sw_small(const Item* __restrict__ items, Item one, SwGeom g, int n_steps, int* err, Rec... rec) {
    constexpr bool MEAS = sizeof...(Rec) != 0;
    extern __shared__ int s_lab[];
    __shared__ int s_bad;
    const Item& it = items ? items[blockIdx.x] : one;
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    using Bonds = SwStoredBonds;
    const int depth = g.depth, rows = g.rows, cols = g.cols, pz = g.pz, pr = g.pr, pc = g.pc;
    const long long pitch = g.pitch;
    const int nrows = depth * rows, n = nrows * cols, tid = threadIdx.x, nt = blockDim.x;
    int8_t* const s_spin = reinterpret_cast<int8_t*>(s_lab + (MEAS ? 2 : 1) * n);
    unsigned* const s_cnt = reinterpret_cast<unsigned*>(s_lab + n);  // MEAS only
    unsigned long long* const s_row = sw_small_scratch<MEAS>();
    unsigned* const s_fz = MEAS ? reinterpret_cast<unsigned*>(s_row + 6) : nullptr;
    if constexpr (MEAS)
        if (tid < 7) s_row[tid] = 0;
    if (tid == 0) s_bad = 0;
    for (int i = tid; i < n; i += nt) {
        const int rho = i / cols, c = i - rho * cols;
        s_spin[i] = it.s[(long long)rho * pitch + c];
    }
    const int hc = (cols + 1) >> 1, npairs = nrows * hc;
    for (int s = 0; s < n_steps; ++s) {
        const uint32_t t = it.k.t + (uint32_t)s;
        for (int i = tid; i < n; i += nt) {
            s_lab[i] = i;
            if constexpr (MEAS) s_cnt[i] = 0;
        }
        __syncthreads();
        int budget = kBudget;
        for (int p = tid; p < npairs; p += nt) {
            const int rho = p / hc, cp = p - rho * hc;
            const int z = rho / rows, r = rho - z * rows;
            const u32x4 w = tsu_philox((uint32_t)cp, (uint32_t)rho, t, it.k.tag_bond, it.k.k0, it.k.k1);
            const u32x4 wl = tsu_philox((uint32_t)cp >> 1, (uint32_t)rho, t, it.k.tag_layer, it.k.k0, it.k.k1);
            const int rd = r + 1 < rows ? rho + 1 : (pr ? z * rows : -1);      // global row of the down neighbour
            const int rf = z + 1 < depth ? rho + rows : (pz ? r : -1);         // ... of the layer neighbour
            u32x4 wg = {0u, 0u, 0u, 0u};  // the ghost bonds' block, drawn once a site of the pair has h s > 0
            bool have_wg = false;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = 2 * cp + j;
                if (c >= cols) break;
                const int i = rho * cols + c, si = s_spin[i];
                const long long e = (long long)rho * pitch + c;
                const int cr = c + 1 < cols ? c + 1 : (pc ? 0 : -1);
                const float h = GHOST ? it.b.h[e] : 0.0f;  // read ahead of the unions, whose atomics it would otherwise wait behind
                if (cr >= 0 && it.b.on(it.b.jr[e], si, s_spin[rho * cols + cr], j ? w.z : w.x))
                    if (!uf_union<GHOST, WG>(s_lab, i, rho * cols + cr, budget)) s_bad = 1;
                if (rd >= 0 && it.b.on(it.b.jd[e], si, s_spin[rd * cols + c], j ? w.w : w.y))
                    if (!uf_union<GHOST, WG>(s_lab, i, rd * cols + c, budget)) s_bad = 1;
                if (rf >= 0 && it.b.on(it.b.jl[e], si, s_spin[rf * cols + c], word_of(wl, c & 3)))
                    if (!uf_union<GHOST, WG>(s_lab, i, rf * cols + c, budget)) s_bad = 1;
                if constexpr (GHOST) {
                    if (Bonds::sat(h, si, 1)) {
                        if (!have_wg) wg = tsu_philox((uint32_t)cp >> 1, (uint32_t)rho, t, it.k.tag_ghost, it.k.k0, it.k.k1);
                        have_wg = true;
                        if (it.b.on(h, si, 1, word_of(wg, c & 3)))
                            if (!uf_union<true, WG>(s_lab, i, -1, budget)) s_bad = 1;
                    }
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < n; i += nt) {
            budget = kBudget;
            const int root = uf_find<GHOST, WG>(s_lab, i, budget);
            if (budget < 0) s_bad = 1;
            if constexpr (MEAS) sw_tally(s_cnt, s_fz, budget >= 0, root, s_spin[i]);
            if (GHOST && root < 0) continue;  // frozen: no coin
            const int rr = root / cols, rc = root - rr * cols;
            if (flip_bit(rr, rc, t, it.k.tag_flip, it.k.k0, it.k.k1)) s_spin[i] = (int8_t)-s_spin[i];
        }
        __syncthreads();
        if (s_bad) break;
        if constexpr (MEAS) sw_small_row(s_lab, s_cnt, s_fz, s_row, n, sw_rec_rows(rec...) + 8 * (long long)s);
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

// tile blockIdx.x (row-major over nz x nr x nc) of tz x tr x tc sites; bonds with both ends in the tile, none across its faces
// or a wrap.  LDS: tz*tr*tc int32 labels (tile-local, row-major: the same order as the global indices inside a tile) and as many
// spins.  Writes the global index of every site's tile root; GHOST: the ghost bond of every site of the tile too, and -1 where the
// tile root is frozen.
template <bool GHOST>
__global__ __launch_bounds__(kSwMaxThreads) void k8_sw_local(Params p) {
    extern __shared__ int s_lab[];
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    using Bonds = SwStoredBonds;
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
        s_spin[i] = (lz < tz && lr < tr && lc < tc) ? p.s[((long long)(z0 + lz) * p.g.rows + r0 + lr) * p.g.pitch + c0 + lc] : (int8_t)0;
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
        const u32x4 wl = tsu_philox((uint32_t)(c0 + lc0) >> 2, (uint32_t)rho, p.k.t, p.k.tag_layer, p.k.k0, p.k.k1);
        u32x4 wg = {0u, 0u, 0u, 0u};
        bool have_wg = false;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int lc = lc0 + j;
            if (lc >= tc) break;
            const int i = (lz * TR + lr) * TC + lc, si = s_spin[i];
            const long long g = rho * p.g.pitch + c0 + lc;
            const float h = GHOST ? p.b.h[g] : 0.0f;  // read ahead of the unions, whose atomics it would otherwise wait behind
            if (lc + 1 < tc && p.b.on(p.b.jr[g], si, s_spin[i + 1], j ? w.z : w.x))
                bad |= !uf_union<GHOST, WG>(s_lab, i, i + 1, budget);
            if (lr + 1 < tr && p.b.on(p.b.jd[g], si, s_spin[i + TC], j ? w.w : w.y))
                bad |= !uf_union<GHOST, WG>(s_lab, i, i + TC, budget);
            if (lz + 1 < tz && p.b.on(p.b.jl[g], si, s_spin[i + TR * TC], word_of(wl, (c0 + lc) & 3)))
                bad |= !uf_union<GHOST, WG>(s_lab, i, i + TR * TC, budget);
            if constexpr (GHOST) {
                if (Bonds::sat(h, si, 1)) {
                    if (!have_wg) wg = tsu_philox((uint32_t)(c0 + lc0) >> 2, (uint32_t)rho, p.k.t, p.k.tag_ghost, p.k.k0, p.k.k1);
                    have_wg = true;
                    if (p.b.on(h, si, 1, word_of(wg, (c0 + lc) & 3)))
                        bad |= !uf_union<true, WG>(s_lab, i, -1, budget);
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += nt) {
        const int lz = i / (TR * TC), rem = i - lz * TR * TC, lr = rem / TC, lc = rem - lr * TC;
        if (lz >= tz || lr >= tr || lc >= tc) continue;
        budget = kBudget;
        const int root = uf_find<GHOST, WG>(s_lab, i, budget);
        bad |= budget < 0;
        const int rz = root / (TR * TC), rrem = root - rz * TR * TC, rr = rrem / TC, rc = rrem - rr * TC;
        const int label = ((z0 + rz) * p.g.rows + r0 + rr) * p.g.cols + c0 + rc;
        p.labels[((long long)(z0 + lz) * p.g.rows + r0 + lr) * p.g.cols + c0 + lc] = (GHOST && root < 0) ? -1 : label;
    }
    if (bad) raise_err(p.err);
}

// one lane per bond across a tile face or a wrap (sw_seam: column seams, row seams, layer seams).  GHOST: either label may be -1 (a
// frozen tile root); joining it with a free root freezes that root's tree
template <bool GHOST>
__global__ __launch_bounds__(256) void k8_sw_merge(Params p) {
    long long rho, rho2;
    int c, c2;
    const int axis = sw_seam<3>(p.g, (long long)blockIdx.x * 256 + threadIdx.x, rho, c, rho2, c2);
    if (axis < 0) return;
    const int sa = p.s[rho * p.g.pitch + c], sb = p.s[rho2 * p.g.pitch + c2];
    const float J = (axis == 0 ? p.b.jr : (axis == 1 ? p.b.jd : p.b.jl))[rho * p.g.pitch + c];
    if (!SwStoredBonds::sat(J, sa, sb)) return;
    uint32_t u;
    if (axis == 2) {
        u = word_of(tsu_philox((uint32_t)c >> 2, (uint32_t)rho, p.k.t, p.k.tag_layer, p.k.k0, p.k.k1), c & 3);
    } else {
        u = word_of(tsu_philox((uint32_t)c >> 1, (uint32_t)rho, p.k.t, p.k.tag_bond, p.k.k0, p.k.k1), 2 * (c & 1) + axis);
    }
    if (!p.b.on(J, sa, sb, u)) return;
    int budget = kBudget;
    const int a = p.labels[rho * p.g.cols + c], b = p.labels[rho2 * p.g.cols + c2];
    if (!uf_union<GHOST, __HIP_MEMORY_SCOPE_AGENT>(p.labels, a, b, budget)) raise_err(p.err);
}

template <bool GHOST>
__global__ __launch_bounds__(256) void k8_sw_resolve(Params p, int quads) {
    sw_resolve<3, GHOST>(p, quads);
}

// GHOST = false: the zero-field entry points (a stored field is refused); true: the ghost-spin ones
template <bool GHOST>
struct K8 {
    static constexpr int DIM = 3;
    using Lattice = tsu_ising3d;
    using Bonds = SwStoredBonds;
    struct Model {
        double T;
    };
    static constexpr const char* who = "ising3d_cluster";
    static constexpr bool refuse_twice = true;
    static constexpr auto small = k8_sw_small<GHOST>;
    static constexpr auto small_measured = k8_sw_small<GHOST, SwRecOut>;
    static constexpr auto local = k8_sw_local<GHOST>;
    static constexpr auto merge = k8_sw_merge<GHOST>;
    static constexpr auto resolve = k8_sw_resolve<GHOST>;

    static int check_model(Lattice* L, const Model& m) {
        tsu_ctx* ctx = L->ctx;
        const long long sites = (long long)L->depth * L->rows * L->cols;
        TSU_REQUIRE(ctx, L->have_disorder, "ising3d_cluster_sweep: call tsu_ising3d_set_disorder first");
        TSU_REQUIRE(ctx, m.T > 0.0 && isfinite(m.T), "Temperature must be positive");
        if (L->have_field && !GHOST)
            return tsu_fail(ctx, TSU_E_UNSUPPORTED, "ising3d_cluster: Swendsen-Wang cluster steps need zero field (a field would need a ghost spin)");
        if (sites >= (1ll << 31)) return tsu_fail(ctx, TSU_E_UNSUPPORTED, "ising3d_cluster: %lld sites exceed 32-bit labels", sites);
        return TSU_OK;
    }
    static int check_err(Lattice* L) { return ising3d_check_err(L); }
    static SwGeom geom(const Lattice* L) {
        SwGeom g = {};
        g.pitch = (long long)L->pitch;
        g.depth = L->depth;
        g.rows = L->rows;
        g.cols = L->cols;
        g.pz = L->pz;
        g.pr = L->pr;
        g.pc = L->pc;
        return g;
    }
    static int8_t* spins(const Lattice* L) { return L->s; }
    static Bonds bonds(const Lattice* L, const Model& m) {
        const size_t plane = (size_t)L->depth * L->rows * L->pitch;
        return Bonds{L->d_dis, L->d_dis + plane, L->d_dis + 2 * plane, L->d_dis + 3 * plane, m.T};  // h: zeros when no field was given
    }
    static bool tile_forced() { return sw3d_tile_forced(); }
    // TSU_SW3D_TILE and the default tile: sw_host.h (sw3d_tile), shared with the 3-D Potts lattice
    static int tile(Lattice* L, SwGeom& g) { return sw3d_tile(L->ctx, L->depth, L->rows, L->cols, g); }
    static int local_threads(const SwGeom& g) { return sw_threads((g.tz * g.tr * g.tc + 15) / 16); }
    static int grow_labels(Lattice* L, size_t bytes) {
        const hipError_t e = ising2d_grow(L->sw.d_labels, L->sw.labels_cap, bytes);
        if (e == hipSuccess) return TSU_OK;
        (void)hipGetLastError();
        return tsu_fail(L->ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "ising3d_cluster: the labels buffer: %s (%zu bytes)",
                        hipGetErrorString(e), bytes);
    }
};

template <bool GHOST>
int sweep_batch(tsu_ising3d* const* lats, int n_lats, int n_steps, const double* Ts, const uint64_t* seeds, const uint32_t* step0s,
                const uint32_t* replicas) {
    if (!lats || n_lats < 1 || !lats[0]) return TSU_E_INVALID;
    TSU_REQUIRE(lats[0]->ctx, Ts && seeds && step0s && replicas, "ising3d_cluster_sweep_batch: Ts, seeds, step0s and replicas are per-lattice arrays");
    return sw_sweep_batch<K8<GHOST>>(lats, n_lats, n_steps, [&](int i) { return typename K8<GHOST>::Model{Ts[i]}; }, seeds, step0s, replicas);
}

}  // namespace

int ising3d_check_err(tsu_ising3d* L) {
    if (L->h_err && *L->h_err) {
        *L->h_err = 0;
        return tsu_fail(L->ctx, TSU_E_HIP, "ising3d: a cluster kernel's union / find loop hit its iteration cap; results invalid");
    }
    return TSU_OK;
}

extern "C" {

int tsu_ising3d_cluster_sweep(tsu_ising3d* L, double T, int n_steps, uint64_t seed, uint32_t step0, uint32_t replica) {
    TSU_ENTER(L ? L->ctx : nullptr);
    return sw_sweep<K8<false>>(L, {T}, n_steps, seed, step0, replica);
}

int tsu_ising3d_cluster_sweep_batch(tsu_ising3d* const* lats, int n_lats, int n_steps, const double* Ts, const uint64_t* seeds,
                                    const uint32_t* step0s, const uint32_t* replicas) {
    TSU_ENTER((lats && n_lats > 0 && lats[0]) ? lats[0]->ctx : nullptr);
    return sweep_batch<false>(lats, n_lats, n_steps, Ts, seeds, step0s, replicas);
}

int tsu_ising3d_cluster_sweep_field(tsu_ising3d* L, double T, int n_steps, uint64_t seed, uint32_t step0, uint32_t replica) {
    TSU_ENTER(L ? L->ctx : nullptr);
    return sw_sweep<K8<true>>(L, {T}, n_steps, seed, step0, replica);
}

int tsu_ising3d_cluster_sweep_field_batch(tsu_ising3d* const* lats, int n_lats, int n_steps, const double* Ts, const uint64_t* seeds,
                                          const uint32_t* step0s, const uint32_t* replicas) {
    TSU_ENTER((lats && n_lats > 0 && lats[0]) ? lats[0]->ctx : nullptr);
    return sweep_batch<true>(lats, n_lats, n_steps, Ts, seeds, step0s, replicas);
}

int tsu_ising3d_cluster_launch_count(tsu_ising3d* L, uint64_t* n) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L || !n) return TSU_E_INVALID;
    *n = L->sw.launches;
    return TSU_OK;
}

int tsu_ising3d_cluster_measure(tsu_ising3d* L, int on) {
    TSU_ENTER(L ? L->ctx : nullptr);
    return sw_measure<K8<false>>(L, on);
}

int tsu_ising3d_cluster_record(tsu_ising3d* L, int64_t* rows, int max_rows, int* n_rows) {
    TSU_ENTER(L ? L->ctx : nullptr);
    return sw_record<K8<false>>(L, rows, max_rows, n_rows);
}

}  // extern "C"

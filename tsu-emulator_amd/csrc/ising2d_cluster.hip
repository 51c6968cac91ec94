// ising2d_cluster.hip -- K6: Swendsen-Wang cluster steps on the lattice handle (gfx950).
//
// One step at zero field: bonds -> connected components -> one coin per component.
//   bond    right bond of site (r, c) (to c + 1, or to 0 across the wrap of a periodic lattice) and its down bond: active iff
//           J s s' > 0 and W[2 (c & 1)] (right) / W[2 (c & 1) + 1] (down) < thr, W = Philox(c >> 1, r, t, TAG_SW_BOND | rep << 8)
//   labels  union-find with min-index roots: a parent always has a smaller index than its child (links are made by atomicMin
//           only), so the root of a finished tree is its component's smallest site index whatever order the atomics ran in
//   flip    the cluster rooted at (r, c) flips iff bit 31 of word c & 3 of Philox(c >> 2, r, t, TAG_SW_FLIP | rep << 8) is set
// Two routes, the same counters and hence the same spins:
//   k6_small   a whole lattice of at most 16384 sites in one workgroup's LDS (spins and labels) for all steps of a call;
//              workgroup b of a launch runs lattice b of a batch
//   k6_local   one workgroup per tile (64 x 64 sites): the tile's bonds and union-find in LDS, tile-root labels to HBM
//   k6_merge   one lane per bond that crosses a tile edge or wraps: union of the two roots in HBM (agent-scope atomicMin)
//   k6_resolve one lane per 4 sites: label -> root, the root's coin, the spin rewritten in place (pad bytes stay 0)
// Every union / find loop draws on a per-lane budget; when it runs out the kernel raises h_err = 2 and gives up on that bond
// instead of spinning (the next synchronising call of the handle reports it).
// Shared with K8's cluster steps (ising3d_cluster.hip): the structs, the uniform-J bond policy's place beside the stored-coupling
// one, the seam decoder, the root chase and the resolve pass (sw_dev.h, DIM = 2: no z term is compiled) and the whole host side
// (sw_host.h, with the traits below).  This file keeps what only K6 has: the threshold from J and T, the whole-lattice check,
// TSU_SW_TILE, the entry points, and the bodies of the kernels that run a union-find (k6_small, k6_local, k6_merge: sw_dev.h says
// why).
#include <math.h>
#include <stdlib.h>

#include "sw_host.h"

namespace {

constexpr int kTile = 64;  // default tile edge of the multi-tile route
constexpr int kLocalThreads = 256;

using Item = SwItem<SwUniformBonds>;
using Params = SwParams<SwUniformBonds>;

// Rec: nothing (k6_small<>: the plain kernel, its arguments and code as they always were) or one SwRecOut (the measured
// instantiation of tsu_hip_cluster_measure.h: one more dword of LDS a site for the roots' counts, a row per step)
template <class... Rec>
__global__ __launch_bounds__(kSwMaxThreads) void k6_small(const Item* __restrict__ items, Item one, SwGeom g, int n_steps, int* err, Rec... rec) {
    constexpr bool MEAS = sizeof...(Rec) != 0;
    extern __shared__ int s_lab[];
    __shared__ int s_bad;
    const Item& it = items ? items[blockIdx.x] : one;
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    const int rows = g.rows, cols = g.cols, periodic = g.pr;
    const int n = rows * cols, tid = threadIdx.x, nt = blockDim.x;
    int8_t* const s_spin = reinterpret_cast<int8_t*>(s_lab + (MEAS ? 2 : 1) * n);
    unsigned* const s_cnt = reinterpret_cast<unsigned*>(s_lab + n);  // MEAS only
    unsigned long long* const s_row = sw_small_scratch<MEAS>();
    unsigned* const s_fz = MEAS ? reinterpret_cast<unsigned*>(s_row + 6) : nullptr;
    if constexpr (MEAS)
        if (tid < 7) s_row[tid] = 0;
    if (tid == 0) s_bad = 0;
    for (int i = tid; i < n; i += nt) {
        const int r = i / cols, c = i - r * cols;
        s_spin[i] = it.s[(long long)r * g.pitch + c];
    }
    const int hc = (cols + 1) >> 1, npairs = rows * hc;
    for (int s = 0; s < n_steps; ++s) {
        const uint32_t t = it.k.t + (uint32_t)s;
        for (int i = tid; i < n; i += nt) {
            s_lab[i] = i;
            if constexpr (MEAS) s_cnt[i] = 0;
        }
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
                if (cr >= 0 && it.b.on(it.b.jsign, si, s_spin[r * cols + cr], j ? w.z : w.x))
                    if (!uf_union<false, WG>(s_lab, i, r * cols + cr, budget)) s_bad = 1;
                if (rd >= 0 && it.b.on(it.b.jsign, si, s_spin[rd * cols + c], j ? w.w : w.y))
                    if (!uf_union<false, WG>(s_lab, i, rd * cols + c, budget)) s_bad = 1;
            }
        }
        __syncthreads();
        for (int i = tid; i < n; i += nt) {
            budget = kBudget;
            const int root = uf_find<false, WG>(s_lab, i, budget);
            if (budget < 0) s_bad = 1;
            if constexpr (MEAS) sw_tally(s_cnt, s_fz, budget >= 0, root, s_spin[i]);
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
        const int r = i / cols, c = i - r * cols;
        it.s[(long long)r * g.pitch + c] = s_spin[i];
    }
}

__global__ __launch_bounds__(kLocalThreads) void k6_local(Params p) {
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
        s_spin[i] = (lr < th && lc < tw) ? p.s[(long long)(r0 + lr) * p.g.pitch + c0 + lc] : (int8_t)0;
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
            if (lc + 1 < tw && p.b.on(p.b.jsign, si, s_spin[i + 1], j ? w.z : w.x)) bad |= !uf_union<false, WG>(s_lab, i, i + 1, budget);
            if (lr + 1 < th && p.b.on(p.b.jsign, si, s_spin[i + TW], j ? w.w : w.y)) bad |= !uf_union<false, WG>(s_lab, i, i + TW, budget);
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

// one lane per bond across a tile edge or the wrap (sw_seam: the vertical seams' right bonds, then the horizontal seams' down bonds)
__global__ __launch_bounds__(256) void k6_merge(Params p) {
    int r, c, r2, c2;
    const int axis = sw_seam<2>(p.g, (long long)blockIdx.x * 256 + threadIdx.x, r, c, r2, c2);
    if (axis < 0) return;
    const int sa = p.s[(long long)r * p.g.pitch + c], sb = p.s[(long long)r2 * p.g.pitch + c2];
    if (!SwUniformBonds::sat(p.b.jsign, sa, sb)) return;
    const u32x4 w = tsu_philox((uint32_t)c >> 1, (uint32_t)r, p.k.t, p.k.tag_bond, p.k.k0, p.k.k1);
    const uint32_t u = axis ? ((c & 1) ? w.w : w.y) : ((c & 1) ? w.z : w.x);
    if ((uint64_t)u >= p.b.thr) return;
    int budget = kBudget;
    const int a = p.labels[(long long)r * p.g.cols + c], b = p.labels[(long long)r2 * p.g.cols + c2];
    if (!uf_union<false, __HIP_MEMORY_SCOPE_AGENT>(p.labels, a, b, budget)) raise_err(p.err);
}

__global__ __launch_bounds__(256) void k6_resolve(Params p, int quads) { sw_resolve<2, false>(p, quads); }

uint64_t threshold(double J, double T) {
    const double p = -expm1(-2.0 * fabs(J) / T);
    return (uint64_t)floor(p * 4294967296.0);
}

// TSU_SW_TILE=<edge> (tests only, read per call): tiles of edge x edge sites, and every lattice on the multi-tile route
int tile_switch() {
    const char* e = getenv("TSU_SW_TILE");
    return e ? atoi(e) : 0;
}

struct K6 {
    static constexpr int DIM = 2;
    using Lattice = tsu_ising2d;
    using Bonds = SwUniformBonds;
    struct Model {
        double J, T;
    };
    static constexpr const char* who = "ising2d_cluster";
    static constexpr bool refuse_twice = false;
    static constexpr auto small = k6_small<>;
    static constexpr auto small_measured = k6_small<SwRecOut>;
    static constexpr auto local = k6_local;
    static constexpr auto merge = k6_merge;
    static constexpr auto resolve = k6_resolve;

    static int check_model(Lattice* L, const Model& m) {
        tsu_ctx* ctx = L->ctx;
        if (!(L->ghost == 0 && L->total_rows == L->rows && L->row0 == 0))
            return tsu_fail(ctx, TSU_E_UNSUPPORTED, "ising2d_cluster: whole lattices only (a slab would need a cluster merge across ranks)");
        TSU_REQUIRE(ctx, m.T > 0.0, "Temperature must be positive");
        TSU_REQUIRE(ctx, isfinite(m.J), "ising2d_cluster: J must be finite");
        return TSU_OK;
    }
    static int check_err(Lattice* L) { return ising2d_check_err(L); }
    static SwGeom geom(const Lattice* L) {
        SwGeom g = {};
        g.pitch = (long long)L->pitch;
        g.depth = 1;
        g.rows = L->rows;
        g.cols = L->cols;
        g.pr = g.pc = L->periodic;
        return g;
    }
    static int8_t* spins(const Lattice* L) { return L->alloc[L->cur]; }
    static Bonds bonds(const Lattice*, const Model& m) { return Bonds{threshold(m.J, m.T), m.J > 0.0 ? 1 : (m.J < 0.0 ? -1 : 0)}; }
    static bool tile_forced() { return tile_switch() != 0; }
    static int tile(Lattice* L, SwGeom& g) {
        tsu_ctx* ctx = L->ctx;
        int edge = tile_switch();
        if (edge <= 0) edge = kTile;
        TSU_REQUIRE(ctx, edge >= 2 && edge <= 64 && (edge & 1) == 0, "TSU_SW_TILE must be an even edge in [2, 64] (got %d)", edge);
        const size_t sites = (size_t)L->rows * L->cols;
        TSU_REQUIRE(ctx, sites < (1ull << 31), "ising2d_cluster: %zu sites exceed 32-bit labels", sites);
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

}  // namespace

extern "C" {

int tsu_ising2d_cluster_threshold(double J, double T, uint64_t* thr) {
    if (!thr || !(T > 0.0) || !isfinite(J)) return TSU_E_INVALID;
    *thr = threshold(J, T);
    return TSU_OK;
}

int tsu_ising2d_cluster_sweep(tsu_ising2d* L, double J, double T, int n_steps, uint64_t seed, uint32_t step0, uint32_t replica) {
    TSU_ENTER(L ? L->ctx : nullptr);
    return sw_sweep<K6>(L, K6::Model{J, T}, n_steps, seed, step0, replica);
}

int tsu_ising2d_cluster_sweep_batch(tsu_ising2d* const* lats, int n_lats, int n_steps, const double* Js, const double* Ts,
                                    const uint64_t* seeds, const uint32_t* step0s, const uint32_t* replicas) {
    TSU_ENTER((lats && n_lats > 0 && lats[0]) ? lats[0]->ctx : nullptr);
    if (!lats || n_lats < 1 || !lats[0]) return TSU_E_INVALID;
    TSU_REQUIRE(lats[0]->ctx, Js && Ts && seeds && step0s && replicas, "ising2d_cluster_sweep_batch: Js, Ts, seeds, step0s and replicas are per-lattice arrays");
    return sw_sweep_batch<K6>(lats, n_lats, n_steps, [&](int i) { return K6::Model{Js[i], Ts[i]}; }, seeds, step0s, replicas);
}

int tsu_ising2d_cluster_launch_count(tsu_ising2d* L, uint64_t* n) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L || !n) return TSU_E_INVALID;
    *n = L->sw.launches;
    return TSU_OK;
}

int tsu_ising2d_cluster_measure(tsu_ising2d* L, int on) {
    TSU_ENTER(L ? L->ctx : nullptr);
    return sw_measure<K6>(L, on);
}

int tsu_ising2d_cluster_record(tsu_ising2d* L, int64_t* rows, int max_rows, int* n_rows) {
    TSU_ENTER(L ? L->ctx : nullptr);
    return sw_record<K6>(L, rows, max_rows, n_rows);
}

}  // extern "C"

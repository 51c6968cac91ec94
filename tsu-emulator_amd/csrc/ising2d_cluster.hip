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
#include <math.h>
#include <stdlib.h>

#include <vector>

#include "ising2d.h"
#include "uf_dev.h"

namespace {

constexpr int kSmallSites = 16384;   // k6_small: rows * cols at most this (80 KB of LDS)
constexpr int kSmallThreads = 1024;
constexpr int kTile = 64;            // default tile edge of the multi-tile route
constexpr int kLocalThreads = 256;

// J s s' > 0 and u < thr (thr may be 2^32: 64-bit compare)
__device__ __forceinline__ bool bond_on(int jsign, int sa, int sb, uint32_t u, uint64_t thr) {
    return jsign * sa * sb > 0 && (uint64_t)u < thr;
}

// ---------------------------------------------------------------- one workgroup per lattice
struct SwItem {
    int8_t* buf;  // row 0
    long long pitch;
    uint64_t thr;
    int jsign;
    uint32_t k0, k1, tag_bond, tag_flip, step0;
};

__global__ __launch_bounds__(kSmallThreads) void k6_small(const SwItem* __restrict__ items, SwItem one, int rows, int cols,
                                                           int periodic, int n_steps, int* err) {
    extern __shared__ int s_lab[];
    __shared__ int s_bad;
    const SwItem& it = items ? items[blockIdx.x] : one;
    const int n = rows * cols, tid = threadIdx.x, nt = blockDim.x;
    int8_t* const s_spin = reinterpret_cast<int8_t*>(s_lab + n);
    if (tid == 0) s_bad = 0;
    for (int i = tid; i < n; i += nt) {
        const int r = i / cols, c = i - r * cols;
        s_spin[i] = it.buf[(long long)r * it.pitch + c];
    }
    const int hc = (cols + 1) >> 1, npairs = rows * hc;
    for (int s = 0; s < n_steps; ++s) {
        const uint32_t t = it.step0 + (uint32_t)s;
        for (int i = tid; i < n; i += nt) s_lab[i] = i;
        __syncthreads();
        int budget = kBudget;
        for (int p = tid; p < npairs; p += nt) {
            const int r = p / hc, cp = p - r * hc;
            const u32x4 w = tsu_philox((uint32_t)cp, (uint32_t)r, t, it.tag_bond, it.k0, it.k1);
            const int rd = r + 1 < rows ? r + 1 : (periodic ? 0 : -1);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = 2 * cp + j;
                if (c >= cols) break;
                const int i = r * cols + c, si = s_spin[i];
                const int cr = c + 1 < cols ? c + 1 : (periodic ? 0 : -1);
                if (cr >= 0 && bond_on(it.jsign, si, s_spin[r * cols + cr], j ? w.z : w.x, it.thr))
                    if (!uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, i, r * cols + cr, budget)) s_bad = 1;
                if (rd >= 0 && bond_on(it.jsign, si, s_spin[rd * cols + c], j ? w.w : w.y, it.thr))
                    if (!uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, i, rd * cols + c, budget)) s_bad = 1;
            }
        }
        __syncthreads();
        for (int i = tid; i < n; i += nt) {
            budget = kBudget;
            const int root = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, i, budget);
            if (budget < 0) s_bad = 1;
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
        const int r = i / cols, c = i - r * cols;
        it.buf[(long long)r * it.pitch + c] = s_spin[i];
    }
}

// ---------------------------------------------------------------- multi-tile route
struct SwParams {
    int8_t* spins;  // row 0
    int* labels;    // rows * cols
    long long pitch;
    int rows, cols, periodic;
    int th, tw, tiles_x, tiles_y;
    uint64_t thr;
    int jsign;
    uint32_t k0, k1, tag_bond, tag_flip, t;
    int* err;
};

// tile blockIdx.x (row-major over tiles_y x tiles_x) of th x tw sites (tw even: a Philox block never straddles two tiles); bonds with both ends in
// the tile, none across its edges or the wrap.  LDS: th*tw int32 labels (tile-local, row-major: the same order as global
// indices inside a tile) and th*tw spins.  Writes the global index of every site's tile root.
__global__ __launch_bounds__(kLocalThreads) void k6_local(SwParams p) {
    extern __shared__ int s_lab[];
    const int TH = p.th, TW = p.tw, n = TH * TW;
    int8_t* const s_spin = reinterpret_cast<int8_t*>(s_lab + n);
    const int ty = (int)(blockIdx.x / (unsigned)p.tiles_x), tx = (int)blockIdx.x - ty * p.tiles_x;
    const int r0 = ty * TH, c0 = tx * TW;
    const int th = p.rows - r0 < TH ? p.rows - r0 : TH, tw = p.cols - c0 < TW ? p.cols - c0 : TW;
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += kLocalThreads) {
        const int lr = i / TW, lc = i - lr * TW;
        s_lab[i] = i;
        s_spin[i] = (lr < th && lc < tw) ? p.spins[(long long)(r0 + lr) * p.pitch + c0 + lc] : (int8_t)0;
    }
    __syncthreads();
    int budget = kBudget;
    bool bad = false;
    const int hw = TW >> 1;
    for (int q = tid; q < TH * hw; q += kLocalThreads) {
        const int lr = q / hw, lc0 = 2 * (q - lr * hw);
        if (lr >= th || lc0 >= tw) continue;
        const u32x4 w = tsu_philox((uint32_t)(c0 + lc0) >> 1, (uint32_t)(r0 + lr), p.t, p.tag_bond, p.k0, p.k1);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int lc = lc0 + j;
            if (lc >= tw) break;
            const int i = lr * TW + lc, si = s_spin[i];
            if (lc + 1 < tw && bond_on(p.jsign, si, s_spin[i + 1], j ? w.z : w.x, p.thr))
                bad |= !uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, i, i + 1, budget);
            if (lr + 1 < th && bond_on(p.jsign, si, s_spin[i + TW], j ? w.w : w.y, p.thr))
                bad |= !uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, i, i + TW, budget);
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += kLocalThreads) {
        const int lr = i / TW, lc = i - lr * TW;
        if (lr >= th || lc >= tw) continue;
        budget = kBudget;
        const int root = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, i, budget);
        bad |= budget < 0;
        const int rr = root / TW, rc = root - rr * TW;
        p.labels[(long long)(r0 + lr) * p.cols + c0 + lc] = (r0 + rr) * p.cols + c0 + rc;
    }
    if (bad) raise_err(p.err);
}

// lanes [0, nv * rows): right bonds of the vertical seams (seam k < tiles_x - 1 at column (k + 1) tw - 1, the last one of a
// periodic lattice at column cols - 1, wrapping to 0); then nh * cols lanes for the down bonds of the horizontal seams
__global__ __launch_bounds__(256) void k6_merge(SwParams p, int nv, int nh) {
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long nvl = (long long)nv * p.rows, total = nvl + (long long)nh * p.cols;
    if (lane >= total) return;
    int r, c, r2, c2;
    bool down;
    if (lane < nvl) {
        const int k = (int)(lane / p.rows);
        r = (int)(lane - (long long)k * p.rows);
        c = k < p.tiles_x - 1 ? (k + 1) * p.tw - 1 : p.cols - 1;
        r2 = r;
        c2 = c + 1 < p.cols ? c + 1 : 0;
        down = false;
    } else {
        const long long l = lane - nvl;
        const int k = (int)(l / p.cols);
        c = (int)(l - (long long)k * p.cols);
        r = k < p.tiles_y - 1 ? (k + 1) * p.th - 1 : p.rows - 1;
        c2 = c;
        r2 = r + 1 < p.rows ? r + 1 : 0;
        down = true;
    }
    const int sa = p.spins[(long long)r * p.pitch + c], sb = p.spins[(long long)r2 * p.pitch + c2];
    if (p.jsign * sa * sb <= 0) return;
    const u32x4 w = tsu_philox((uint32_t)c >> 1, (uint32_t)r, p.t, p.tag_bond, p.k0, p.k1);
    const uint32_t u = down ? ((c & 1) ? w.w : w.y) : ((c & 1) ? w.z : w.x);
    if ((uint64_t)u >= p.thr) return;
    int budget = kBudget;
    const int a = p.labels[(long long)r * p.cols + c], b = p.labels[(long long)r2 * p.cols + c2];
    if (!uf_union<__HIP_MEMORY_SCOPE_AGENT>(p.labels, a, b, budget)) raise_err(p.err);
}

// one lane per 4 sites of a row (one 4-byte load and store; the pad bytes beyond cols are 0 and stay 0): the root of each
// site, the root's coin (one Philox block per distinct root of the lane), the spin rewritten
__global__ __launch_bounds__(256) void k6_resolve(SwParams p, int quads) {
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    const int r = (int)(lane / quads), c0 = 4 * (int)(lane - (long long)r * quads);
    if (r >= p.rows) return;
    int8_t* const row = p.spins + (long long)r * p.pitch;
    uint32_t v = *reinterpret_cast<const uint32_t*>(row + c0);
    int last = -1;
    bool last_flip = false, bad = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (c0 + j >= p.cols) break;
        const long long g = (long long)r * p.cols + c0 + j;
        int x = p.labels[g], budget = kBudget;
        for (int y = p.labels[x]; y != x; y = p.labels[x]) {
            x = y;
            if (--budget < 0) {
                bad = true;
                break;
            }
        }
        if (x != last) {
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
bool whole_lattice(const tsu_ising2d* L) { return L->ghost == 0 && L->total_rows == L->rows && L->row0 == 0; }

// TSU_SW_TILE=<edge> (tests only, read per call): tiles of edge x edge sites, and every lattice on the multi-tile route
int tile_switch() {
    const char* e = getenv("TSU_SW_TILE");
    return e ? atoi(e) : 0;
}

bool small_route(const tsu_ising2d* L) {
    return tile_switch() == 0 && (long long)L->rows * L->cols <= kSmallSites;
}

int check_model(tsu_ctx* ctx, double J, double T) {
    TSU_REQUIRE(ctx, T > 0.0, "Temperature must be positive");
    TSU_REQUIRE(ctx, isfinite(J), "ising2d_cluster: J must be finite");
    return TSU_OK;
}

uint64_t threshold(double J, double T) {
    const double p = -expm1(-2.0 * fabs(J) / T);
    return (uint64_t)floor(p * 4294967296.0);
}

int ensure_err(tsu_ising2d* L, int** d_err) {
    tsu_ctx* ctx = L->ctx;
    if (!L->h_err) {
        TSU_HIP_TRY(ctx, hipHostMalloc(&L->h_err, sizeof(int), hipHostMallocMapped));
        *L->h_err = 0;
    }
    TSU_HIP_TRY(ctx, hipHostGetDevicePointer((void**)d_err, L->h_err, 0));
    return TSU_OK;
}

SwItem make_item(const tsu_ising2d* L, double J, double T, uint64_t seed, uint32_t step0, uint32_t replica) {
    SwItem it;
    it.buf = L->alloc[L->cur];
    it.pitch = (long long)L->pitch;
    it.thr = threshold(J, T);
    it.jsign = J > 0.0 ? 1 : (J < 0.0 ? -1 : 0);
    it.k0 = (uint32_t)seed;
    it.k1 = (uint32_t)(seed >> 32);
    it.tag_bond = TSU_TAG_SW_BOND | (replica << 8);
    it.tag_flip = TSU_TAG_SW_FLIP | (replica << 8);
    it.step0 = step0;
    return it;
}

size_t small_lds(const tsu_ising2d* L) { return (size_t)L->rows * L->cols * 5; }

int small_threads(const tsu_ising2d* L) {
    const long long pairs = (long long)L->rows * ((L->cols + 1) / 2);
    const long long t = (pairs + 63) / 64 * 64;
    return (int)(t < kSmallThreads ? t : kSmallThreads);
}

int run_small(tsu_ising2d* const* lats, int n, const SwItem* items, int n_steps) {
    tsu_ising2d* L0 = lats[0];
    tsu_ctx* ctx = L0->ctx;
    int* d_err = nullptr;
    int rc = ensure_err(L0, &d_err);
    if (rc != TSU_OK) return rc;
    const size_t lds = small_lds(L0);
    TSU_HIP_TRY(ctx, tsu_func_allow_lds(ctx, (const void*)k6_small, (int)lds));
    const SwItem* d_items = nullptr;
    if (n > 1) {
        const size_t bytes = (size_t)n * sizeof(SwItem);
        TSU_HIP_TRY(ctx, ising2d_grow(L0->d_sw_batch, L0->sw_batch_cap, bytes));
        // the host array dies with this call: wait for the copy (a few KB); the launch itself stays asynchronous
        TSU_HIP_TRY(ctx, hipMemcpyAsync(L0->d_sw_batch, items, bytes, hipMemcpyHostToDevice, ctx->stream));
        TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        d_items = (const SwItem*)L0->d_sw_batch;
    }
    hipLaunchKernelGGL(k6_small, dim3((unsigned)n), dim3((unsigned)small_threads(L0)), lds, ctx->stream, d_items, items[0], L0->rows,
                       L0->cols, L0->periodic, n_steps, d_err);
    TSU_HIP_TRY(ctx, hipGetLastError());
    for (int i = 0; i < n; ++i) lats[i]->sw_launches += 1;
    return TSU_OK;
}

int run_tiles(tsu_ising2d* L, const SwItem& it, int n_steps) {
    tsu_ctx* ctx = L->ctx;
    int edge = tile_switch();
    if (edge <= 0) edge = kTile;
    TSU_REQUIRE(ctx, edge >= 2 && edge <= 64 && (edge & 1) == 0, "TSU_SW_TILE must be an even edge in [2, 64] (got %d)", edge);
    const size_t sites = (size_t)L->rows * L->cols;
    TSU_REQUIRE(ctx, sites < (1ull << 31), "ising2d_cluster: %zu sites exceed 32-bit labels", sites);
    TSU_HIP_TRY(ctx, ising2d_grow(L->d_labels, L->labels_cap, sites * sizeof(int32_t)));
    SwParams p;
    p.spins = it.buf;
    p.labels = L->d_labels;
    p.pitch = it.pitch;
    p.rows = L->rows;
    p.cols = L->cols;
    p.periodic = L->periodic;
    p.th = p.tw = edge;
    p.tiles_x = (L->cols + edge - 1) / edge;
    p.tiles_y = (L->rows + edge - 1) / edge;
    p.thr = it.thr;
    p.jsign = it.jsign;
    p.k0 = it.k0;
    p.k1 = it.k1;
    p.tag_bond = it.tag_bond;
    p.tag_flip = it.tag_flip;
    int rc = ensure_err(L, &p.err);
    if (rc != TSU_OK) return rc;
    const int nv = p.tiles_x - 1 + (L->periodic ? 1 : 0), nh = p.tiles_y - 1 + (L->periodic ? 1 : 0);
    const long long merge_lanes = (long long)nv * L->rows + (long long)nh * L->cols;
    const size_t lds = (size_t)edge * edge * 5;
    const int quads = (L->cols + 3) / 4;
    const unsigned tiles = (unsigned)((long long)p.tiles_x * p.tiles_y), resolve_blocks = (unsigned)(((long long)quads * L->rows + 255) / 256);
    for (int s = 0; s < n_steps; ++s) {
        p.t = it.step0 + (uint32_t)s;
        hipLaunchKernelGGL(k6_local, dim3(tiles), dim3(kLocalThreads), lds, ctx->stream, p);
        if (merge_lanes > 0)
            hipLaunchKernelGGL(k6_merge, dim3((unsigned)((merge_lanes + 255) / 256)), dim3(256), 0, ctx->stream, p, nv, nh);
        hipLaunchKernelGGL(k6_resolve, dim3(resolve_blocks), dim3(256), 0, ctx->stream, p, quads);
        L->sw_launches += merge_lanes > 0 ? 3 : 2;
    }
    TSU_HIP_TRY(ctx, hipGetLastError());
    return TSU_OK;
}

int check_call(tsu_ising2d* L, double J, double T, int n_steps, uint32_t step0, uint32_t replica) {
    tsu_ctx* ctx = L->ctx;
    if (!whole_lattice(L))
        return tsu_fail(ctx, TSU_E_UNSUPPORTED, "ising2d_cluster: whole lattices only (a slab would need a cluster merge across ranks)");
    int rc = check_model(ctx, J, T);
    if (rc != TSU_OK) return rc;
    TSU_REQUIRE(ctx, n_steps >= 0, "ising2d_cluster: n_steps must be >= 0");
    TSU_REQUIRE(ctx, (uint64_t)step0 + (uint64_t)n_steps <= (1ull << 32), "ising2d_cluster: step counter overflow");
    TSU_REQUIRE_REPLICA(ctx, replica, "ising2d_cluster");
    return ising2d_check_err(L);  // a cap that expired in an earlier call
}

}  // namespace

extern "C" {

int tsu_ising2d_cluster_threshold(double J, double T, uint64_t* thr) {
    if (!thr || !(T > 0.0) || !isfinite(J)) return TSU_E_INVALID;
    *thr = threshold(J, T);
    return TSU_OK;
}

int tsu_ising2d_cluster_sweep(tsu_ising2d* L, double J, double T, int n_steps, uint64_t seed, uint32_t step0, uint32_t replica) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    int rc = check_call(L, J, T, n_steps, step0, replica);
    if (rc != TSU_OK || n_steps == 0) return rc;
    const SwItem it = make_item(L, J, T, seed, step0, replica);
    return small_route(L) ? run_small(&L, 1, &it, n_steps) : run_tiles(L, it, n_steps);
}

int tsu_ising2d_cluster_sweep_batch(tsu_ising2d* const* lats, int n_lats, int n_steps, const double* Js, const double* Ts,
                                    const uint64_t* seeds, const uint32_t* step0s, const uint32_t* replicas) {
    TSU_ENTER((lats && n_lats > 0 && lats[0]) ? lats[0]->ctx : nullptr);
    if (!lats || n_lats < 1 || !lats[0]) return TSU_E_INVALID;
    tsu_ctx* ctx = lats[0]->ctx;
    TSU_REQUIRE(ctx, Js && Ts && seeds && step0s && replicas, "ising2d_cluster_sweep_batch: Js, Ts, seeds, step0s and replicas are per-lattice arrays");
    bool one_launch = true;  // every lattice on k6_small, all of one shape and boundary
    for (int i = 0; i < n_lats; ++i) {
        tsu_ising2d* L = lats[i];
        TSU_REQUIRE(ctx, L && L->ctx == ctx, "ising2d_cluster_sweep_batch: lattice %d is NULL or belongs to another context", i);
        int rc = check_call(L, Js[i], Ts[i], n_steps, step0s[i], replicas[i]);
        if (rc != TSU_OK) return rc;
        one_launch = one_launch && small_route(L) && L->rows == lats[0]->rows && L->cols == lats[0]->cols && L->periodic == lats[0]->periodic;
    }
    if (n_steps == 0) return TSU_OK;
    if (one_launch) {
        std::vector<SwItem> items((size_t)n_lats);
        for (int i = 0; i < n_lats; ++i) items[(size_t)i] = make_item(lats[i], Js[i], Ts[i], seeds[i], step0s[i], replicas[i]);
        return run_small(lats, n_lats, items.data(), n_steps);
    }
    for (int i = 0; i < n_lats; ++i) {
        int rc = tsu_ising2d_cluster_sweep(lats[i], Js[i], Ts[i], n_steps, seeds[i], step0s[i], replicas[i]);
        if (rc != TSU_OK) return rc;
    }
    return TSU_OK;
}

int tsu_ising2d_cluster_launch_count(tsu_ising2d* L, uint64_t* n) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L || !n) return TSU_E_INVALID;
    *n = L->sw_launches;
    return TSU_OK;
}

}  // extern "C"

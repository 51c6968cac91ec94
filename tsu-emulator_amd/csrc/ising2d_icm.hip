// ising2d_icm.hip -- K7: replica cluster moves (Houdayer's isoenergetic cluster move) inside the tempering ladder (gfx950).
//
// One pass, for every participating slot i (T_i <= t_max), a / b = the walkers of ladder 0 / ladder 1 now at slot i:
//   q       q_x = a_x b_x per site; sites with q = -1 are joined to their right and down lattice neighbours with q = -1 (wrapping
//           on a periodic lattice), whatever J is on that bond; sites with q = +1 belong to no cluster
//   labels  union-find with min-index roots (uf_dev.h): the root of a cluster is its smallest index r * cols + c
//   flip    the cluster rooted at (r, c) flips in BOTH walkers iff bit 31 of word c & 3 of
//           Philox(c >> 2, r, m, TAG_PT_ICM | slot << 8) is set, key = the ladder's seed, m = the handle's cluster-pass counter
// Flipping a q = -1 cluster in both walkers exchanges it between them: E_a + E_b and every q_x stay as they were, so the pass
// is a weight-preserving involution of the pair and needs no accept / reject step.
// Two routes, the same counters and hence the same spins:
//   k7_icm_small    one workgroup per slot, the whole lattice (at most 16384 sites) in LDS: 4 B label + 1 B flags per site
//   k7_icm_local    grid (tiles, slots): q of a tile staged from the two walkers, union-find in LDS, global root per site to HBM
//                   (sites with q = +1 get kNone and cost no union)
//   k7_icm_merge    grid (.., slots): one lane per bond across a tile seam or the wrap, union of the two roots in HBM
//   k7_icm_resolve  grid (.., slots): one lane per 4 sites: label -> root, one coin per distinct root of the lane, the 4 bytes of
//                   both walkers rewritten; clusters and flipped sites counted with one atomic per workgroup
// One launch (small) or three (tiled) per pass whatever the number of slots.  Every union / find loop draws on the per-lane
// budget of uf_dev.h and raises h_err = 2 when it runs out; no kernel waits on another workgroup.
// Shared with the Swendsen-Wang steps (sw_dev.h): the geometry struct, the seam decoder of the merge kernel and the root chase of the
// resolve kernel.  The q-staging, the flags, the statistics and the two-walker stores are this file's own.
#include <cstdlib>

#include "ising2d_pt.h"
#include "sw_dev.h"

namespace {

constexpr int kSmallSites = 16384;  // k7_icm_small: rows * cols at most this (80 KB of LDS), K6's bound
constexpr int kSmallThreads = 1024;
constexpr int kTile = 64;           // default tile edge of the tiled route
constexpr int kLocalThreads = 256;
constexpr int kNone = -1;           // label of a site with q = +1

struct IcmParams {
    int8_t* const* s;      // walker g = ladder * R + w -> row 0 of its spin plane
    const int32_t* was;    // [ladder][slot] -> walker
    const int32_t* slots;  // participating slots (grid index -> slot)
    int32_t* labels;       // tiled route: [grid index][rows * cols]
    long long* stats;      // [3][R]: passes, clusters, flipped
    SwGeom g;              // depth 1, pz 0, pr = pc = periodic; tiles of tr x tc sites on the tiled route
    int R;
    uint32_t k0, k1, m;
    int* err;
};

__device__ __forceinline__ int8_t* walker_plane(const IcmParams& p, int ladder, int slot) {
    return p.s[ladder * p.R + p.was[ladder * p.R + slot]];
}

// ---------------------------------------------------------------- one workgroup per slot
// LDS flags per site: bit 0 = q is -1, bit 1 = this root's coin says flip, bit 2 = a is -1
__global__ __launch_bounds__(kSmallThreads) void k7_icm_small(IcmParams p) {
    extern __shared__ int s_lab[];
    __shared__ int s_bad, s_ncl, s_nfl;
    const int slot = p.slots[blockIdx.x];
    int8_t* const a = walker_plane(p, 0, slot);
    int8_t* const b = walker_plane(p, 1, slot);
    const int rows = p.g.rows, cols = p.g.cols, n = rows * cols, tid = threadIdx.x, nt = blockDim.x;
    uint8_t* const s_q = reinterpret_cast<uint8_t*>(s_lab + n);
    if (tid == 0) s_bad = s_ncl = s_nfl = 0;
    for (int i = tid; i < n; i += nt) {
        const int r = i / cols, c = i - r * cols;
        const long long g = (long long)r * p.g.pitch + c;
        const int sa = a[g], sb = b[g];
        s_q[i] = (uint8_t)((sa * sb < 0 ? 1 : 0) | (sa < 0 ? 4 : 0));
        s_lab[i] = i;
    }
    __syncthreads();
    int budget = kBudget;
    bool bad = false;
    for (int i = tid; i < n; i += nt) {
        if (!(s_q[i] & 1)) continue;
        const int r = i / cols, c = i - r * cols;
        const int cr = c + 1 < cols ? c + 1 : (p.g.pc ? 0 : -1);
        const int rd = r + 1 < rows ? r + 1 : (p.g.pc ? 0 : -1);
        if (cr >= 0 && (s_q[r * cols + cr] & 1)) bad |= !uf_union<false, __HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, i, r * cols + cr, budget);
        if (rd >= 0 && (s_q[rd * cols + c] & 1)) bad |= !uf_union<false, __HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, i, rd * cols + c, budget);
    }
    __syncthreads();
    // every site's label becomes its root (a root is an ancestor: lanes still chasing through this site lose nothing)
    for (int i = tid; i < n; i += nt) {
        if (!(s_q[i] & 1)) continue;
        budget = kBudget;
        const int root = uf_find<false, __HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, i, budget);
        bad |= budget < 0;
        __hip_atomic_store(s_lab + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (s_bad) {
        if (tid == 0) raise_err(p.err);
        return;  // both walkers keep their spins from before the pass
    }
    const uint32_t tag = TSU_TAG_PT_ICM | ((uint32_t)slot << 8);
    int ncl = 0, nfl = 0;
    for (int i = tid; i < n; i += nt) {
        if (!(s_q[i] & 1) || s_lab[i] != i) continue;
        const int r = i / cols, c = i - r * cols;
        ncl += 1;
        if (flip_bit(r, c, p.m, tag, p.k0, p.k1)) s_q[i] |= 2;
    }
    __syncthreads();
    for (int i = tid; i < n; i += nt) {
        const int f = s_q[i];
        if (!(f & 1) || !(s_q[s_lab[i]] & 2)) continue;
        const int r = i / cols, c = i - r * cols;
        const long long g = (long long)r * p.g.pitch + c;
        const int8_t sa = (f & 4) ? (int8_t)-1 : (int8_t)1;  // b = -a here: flipping both exchanges them
        a[g] = (int8_t)-sa;
        b[g] = sa;
        nfl += 1;
    }
    if (ncl) atomicAdd(&s_ncl, ncl);
    if (nfl) atomicAdd(&s_nfl, nfl);
    __syncthreads();
    if (tid == 0) {  // the only workgroup of this slot
        p.stats[slot] += 1;
        p.stats[p.R + slot] += s_ncl;
        p.stats[2 * p.R + slot] += s_nfl;
    }
}

// ---------------------------------------------------------------- tiled route
// tile blockIdx.x (row-major over tiles_y x tiles_x) of th x tw sites of slot blockIdx.y.  LDS: th*tw int32 labels (tile-local,
// row-major: the same order as global indices inside a tile) and th*tw q bytes (1 = q is -1; 0 outside the lattice).
__global__ __launch_bounds__(kLocalThreads) void k7_icm_local(IcmParams p) {
    extern __shared__ int s_lab[];
    const int TH = p.g.tr, TW = p.g.tc, n = TH * TW;
    uint8_t* const s_q = reinterpret_cast<uint8_t*>(s_lab + n);
    const int slot = p.slots[blockIdx.y];
    const int8_t* const a = walker_plane(p, 0, slot);
    const int8_t* const b = walker_plane(p, 1, slot);
    int32_t* const labels = p.labels + (size_t)blockIdx.y * p.g.rows * p.g.cols;
    const int ty = (int)(blockIdx.x / (unsigned)p.g.nc), tx = (int)blockIdx.x - ty * p.g.nc;
    const int r0 = ty * TH, c0 = tx * TW;
    const int th = p.g.rows - r0 < TH ? p.g.rows - r0 : TH, tw = p.g.cols - c0 < TW ? p.g.cols - c0 : TW;
    const int tid = threadIdx.x;
    if ((TW & 3) == 0) {
        // 4 sites per lane: c0 and the pitch are multiples of 4
        const int qw = TW >> 2;
        for (int i4 = tid; i4 < TH * qw; i4 += kLocalThreads) {
            const int lr = i4 / qw, lc = 4 * (i4 - lr * qw);
            uint32_t q = 0;
            if (lr < th && lc < tw) {
                const long long g = (long long)(r0 + lr) * p.g.pitch + c0 + lc;
                const uint32_t va = *reinterpret_cast<const uint32_t*>(a + g), vb = *reinterpret_cast<const uint32_t*>(b + g);
                q = ((va ^ vb) >> 7) & 0x01010101u;  // +1 = 0x01, -1 = 0xFF: bit 7 of the XOR is set iff the two spins differ
                if (lc + 4 > tw) q &= 0xFFFFFFFFu >> (8 * (lc + 4 - tw));  // bytes beyond the last column
            }
            const int i = lr * TW + lc;
            *reinterpret_cast<uint32_t*>(s_q + i) = q;
            s_lab[i] = i;
            s_lab[i + 1] = i + 1;
            s_lab[i + 2] = i + 2;
            s_lab[i + 3] = i + 3;
        }
    } else {
        for (int i = tid; i < n; i += kLocalThreads) {
            const int lr = i / TW, lc = i - lr * TW;
            int q = 0;
            if (lr < th && lc < tw) {
                const long long g = (long long)(r0 + lr) * p.g.pitch + c0 + lc;
                q = (int)a[g] * (int)b[g] < 0;
            }
            s_q[i] = (uint8_t)q;
            s_lab[i] = i;
        }
    }
    __syncthreads();
    int budget = kBudget;
    bool bad = false;
    for (int i = tid; i < n; i += kLocalThreads) {
        if (!s_q[i]) continue;
        const int lr = i / TW, lc = i - lr * TW;
        if (lc + 1 < tw && s_q[i + 1]) bad |= !uf_union<false, __HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, i, i + 1, budget);
        if (lr + 1 < th && s_q[i + TW]) bad |= !uf_union<false, __HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, i, i + TW, budget);
    }
    __syncthreads();
    for (int i = tid; i < n; i += kLocalThreads) {
        const int lr = i / TW, lc = i - lr * TW;
        if (lr >= th || lc >= tw) continue;
        int lab = kNone;
        if (s_q[i]) {
            budget = kBudget;
            const int root = uf_find<false, __HIP_MEMORY_SCOPE_WORKGROUP>(s_lab, i, budget);
            bad |= budget < 0;
            const int rr = root / TW, rc = root - rr * TW;
            lab = (r0 + rr) * p.g.cols + c0 + rc;
        }
        labels[(long long)(r0 + lr) * p.g.cols + c0 + lc] = lab;
    }
    if (bad) raise_err(p.err);
}

// one lane per bond across a tile seam or the wrap (sw_seam: the vertical seams' right bonds, then the horizontal seams' down
// bonds).  A label other than kNone says q = -1 at that site: the spins are not read again.
__global__ __launch_bounds__(256) void k7_icm_merge(IcmParams p) {
    int r, c, r2, c2;
    if (sw_seam<2>(p.g, (long long)blockIdx.x * 256 + threadIdx.x, r, c, r2, c2) < 0) return;
    int32_t* const labels = p.labels + (size_t)blockIdx.y * p.g.rows * p.g.cols;
    const int la = labels[(long long)r * p.g.cols + c], lb = labels[(long long)r2 * p.g.cols + c2];
    if (la == kNone || lb == kNone) return;
    int budget = kBudget;
    if (!uf_union<false, __HIP_MEMORY_SCOPE_AGENT>(labels, la, lb, budget)) raise_err(p.err);
}

// one lane per 4 sites of a row of slot blockIdx.y (one 4-byte load and store per walker; the pad bytes beyond cols are 0 and
// stay 0): the root of each q = -1 site, the root's coin (one Philox block per distinct root of the lane), both walkers' bytes
// negated where it says flip
__global__ __launch_bounds__(256) void k7_icm_resolve(IcmParams p, int quads) {
    __shared__ int s_ncl, s_nfl;
    if (threadIdx.x == 0) s_ncl = s_nfl = 0;
    __syncthreads();
    const int slot = p.slots[blockIdx.y];
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    const int r = (int)(lane / quads), c0 = 4 * (int)(lane - (long long)r * quads);
    int ncl = 0, nfl = 0;
    if (r < p.g.rows) {
        const int32_t* const labels = p.labels + (size_t)blockIdx.y * p.g.rows * p.g.cols;
        const uint32_t tag = TSU_TAG_PT_ICM | ((uint32_t)slot << 8);
        int last = kNone;
        bool last_flip = false, bad = false;
        uint32_t mask = 0;  // 0xFF in the bytes that flip
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (c0 + j >= p.g.cols) break;
            const int g = r * p.g.cols + c0 + j;
            int x = labels[g];
            if (x == kNone) continue;
            ncl += x == g;
            x = sw_chase<false>(labels, x, bad);
            if (x != last) {
                const int rr = x / p.g.cols, rc = x - rr * p.g.cols;
                last = x;
                last_flip = flip_bit(rr, rc, p.m, tag, p.k0, p.k1);
            }
            if (last_flip) {
                mask |= 0xFFu << (8 * j);
                nfl += 1;
            }
        }
        if (mask) {
            // negate the masked bytes: +1 = 0x01 <-> -1 = 0xFF is an XOR with 0xFE
            const long long off = (long long)r * p.g.pitch + c0;
            uint32_t* const pa = reinterpret_cast<uint32_t*>(walker_plane(p, 0, slot) + off);
            uint32_t* const pb = reinterpret_cast<uint32_t*>(walker_plane(p, 1, slot) + off);
            *pa ^= mask & 0xFEFEFEFEu;
            *pb ^= mask & 0xFEFEFEFEu;
        }
        if (bad) raise_err(p.err);
    }
    if (ncl) atomicAdd(&s_ncl, ncl);
    if (nfl) atomicAdd(&s_nfl, nfl);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long*>(p.stats + slot), 1ull);
        if (s_ncl) atomicAdd(reinterpret_cast<unsigned long long*>(p.stats + p.R + slot), (unsigned long long)s_ncl);
        if (s_nfl) atomicAdd(reinterpret_cast<unsigned long long*>(p.stats + 2 * p.R + slot), (unsigned long long)s_nfl);
    }
}

// ---------------------------------------------------------------- host side
// TSU_ICM_TILE=<edge> (tests only, read per call): tiles of edge x edge sites, and every lattice on the tiled route
int tile_switch() {
    const char* e = getenv("TSU_ICM_TILE");
    return e ? atoi(e) : 0;
}

size_t sites_of(const tsu_pt2d* P) { return (size_t)P->lat[0]->rows * P->lat[0]->cols; }

int grow_labels(tsu_pt2d* P) {
    const size_t bytes = sites_of(P) * (size_t)P->icm_n * sizeof(int32_t);
    if (hipError_t e = ising2d_grow(P->d_icm_labels, P->icm_labels_cap, bytes); e != hipSuccess)
        return tsu_fail(P->ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP,
                        "pt2d cluster moves: %zu bytes of labels (%d slots of %zu sites): %s", bytes, P->icm_n, sites_of(P),
                        hipGetErrorString(e));
    return TSU_OK;
}

}  // namespace

int pt2d_icm_slots(tsu_pt2d* P) {
    if (P->icm_every == 0 || !P->have_T) return TSU_OK;
    tsu_ctx* ctx = P->ctx;
    int32_t slots[kPtMaxTemps];
    int n = 0;
    for (int i = 0; i < P->R; ++i)
        if (P->h_T[i] <= P->icm_tmax) slots[n++] = i;
    if (n) TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_icm_slots, slots, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // `slots` goes; an earlier pass is done with the old list
    P->icm_n = n;
    return n && sites_of(P) > (size_t)kSmallSites ? grow_labels(P) : TSU_OK;
}

int pt2d_icm_reset(tsu_pt2d* P) {
    P->icm_passes = 0;
    P->icm_launches = 0;
    if (P->d_icm_stats) {
        TSU_HIP_TRY(P->ctx, hipMemsetAsync(P->d_icm_stats, 0, 3 * (size_t)P->R * sizeof(long long), P->ctx->stream));
        TSU_HIP_TRY(P->ctx, hipStreamSynchronize(P->ctx->stream));
    }
    return TSU_OK;
}

void pt2d_icm_free(tsu_pt2d* P) {
    void* bufs[] = {P->d_icm_slots, P->d_icm_labels, P->d_icm_stats};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    P->d_icm_slots = nullptr;
    P->d_icm_labels = nullptr;
    P->d_icm_stats = nullptr;
    P->icm_labels_cap = 0;
    P->icm_n = 0;
}

int pt2d_icm_enqueue(tsu_pt2d* P) {
    tsu_ctx* ctx = P->ctx;
    const tsu_ising2d* L = P->lat[0];
    const uint32_t m = P->icm_passes;
    P->icm_passes += 1;
    if (P->icm_n == 0) return TSU_OK;
    int edge = tile_switch();
    const bool small = edge == 0 && sites_of(P) <= (size_t)kSmallSites;
    IcmParams p;
    p.s = P->d_s;
    p.was = P->d_was;
    p.slots = P->d_icm_slots;
    p.labels = nullptr;
    p.stats = P->d_icm_stats;
    p.g = SwGeom{};
    p.g.pitch = (long long)L->pitch;
    p.g.depth = 1;
    p.g.rows = L->rows;
    p.g.cols = L->cols;
    p.g.pr = p.g.pc = L->periodic;
    p.R = P->R;
    p.k0 = P->key0;
    p.k1 = P->key1;
    p.m = m;
    int rc = tsu_err_flag(ctx, P->lat[0]->h_err, &p.err);
    if (rc != TSU_OK) return rc;
    const unsigned ns = (unsigned)P->icm_n;
    if (small) {
        const size_t lds = sites_of(P) * 5;
        const size_t t = (sites_of(P) + 63) / 64 * 64;
        TSU_HIP_TRY(ctx, tsu_func_allow_lds(ctx, (const void*)k7_icm_small, (int)lds));
        hipLaunchKernelGGL(k7_icm_small, dim3(ns), dim3((unsigned)(t < (size_t)kSmallThreads ? t : kSmallThreads)), lds, ctx->stream, p);
        P->icm_launches += 1;
    } else {
        if (edge <= 0) edge = kTile;
        TSU_REQUIRE(ctx, edge >= 2 && edge <= 64, "TSU_ICM_TILE must be an edge in [2, 64] (got %d)", edge);
        TSU_REQUIRE(ctx, sites_of(P) < (1ull << 31), "pt2d cluster moves: %zu sites exceed 32-bit labels", sites_of(P));
        rc = grow_labels(P);
        if (rc != TSU_OK) return rc;
        p.labels = P->d_icm_labels;
        p.g.tr = p.g.tc = edge;
        p.g.nc = (L->cols + edge - 1) / edge;
        p.g.nr = (L->rows + edge - 1) / edge;
        const long long merge_lanes = sw_seam_lanes<2>(p.g);
        const size_t lds = (size_t)edge * edge * 5;
        const int quads = (L->cols + 3) / 4;
        const unsigned tiles = (unsigned)((long long)p.g.nc * p.g.nr);
        const unsigned resolve_blocks = (unsigned)(((long long)quads * L->rows + 255) / 256);
        hipLaunchKernelGGL(k7_icm_local, dim3(tiles, ns), dim3(kLocalThreads), lds, ctx->stream, p);
        // a lattice of one tile without a wrap has no seam; the launch stays so that a pass is three launches on this route
        hipLaunchKernelGGL(k7_icm_merge, dim3((unsigned)((merge_lanes + 255) / 256 > 0 ? (merge_lanes + 255) / 256 : 1), ns), dim3(256), 0,
                           ctx->stream, p);
        hipLaunchKernelGGL(k7_icm_resolve, dim3(resolve_blocks, ns), dim3(256), 0, ctx->stream, p, quads);
        P->icm_launches += 3;
    }
    TSU_HIP_TRY(ctx, hipGetLastError());
    return TSU_OK;
}

extern "C" {

int tsu_pt2d_set_cluster_moves(tsu_pt2d* P, int every, double t_max) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, every >= 0, "pt2d_set_cluster_moves: every must be >= 0 (0 switches the move off), got %d", every);
    TSU_REQUIRE(ctx, t_max > 0.0, "pt2d_set_cluster_moves: t_max must be positive (+inf: every slot), got %g", t_max);
    if (every == 0) {
        TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        pt2d_icm_free(P);  // the statistics go with the buffers
        P->icm_every = 0;
        return TSU_OK;
    }
    TSU_REQUIRE(ctx, P->nl == 2, "pt2d_set_cluster_moves: the move exchanges clusters between two ladders; this handle has %d", P->nl);
    if (!P->d_icm_slots) TSU_HIP_TRY(ctx, hipMalloc((void**)&P->d_icm_slots, (size_t)P->R * sizeof(int32_t)));
    if (!P->d_icm_stats) {
        TSU_HIP_TRY(ctx, hipMalloc((void**)&P->d_icm_stats, 3 * (size_t)P->R * sizeof(long long)));
        TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_icm_stats, 0, 3 * (size_t)P->R * sizeof(long long), ctx->stream));
    }
    P->icm_every = every;
    P->icm_tmax = t_max;
    return pt2d_icm_slots(P);
}

int tsu_pt2d_cluster_move(tsu_pt2d* P) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, P->icm_every >= 1, "pt2d_cluster_move: call tsu_pt2d_set_cluster_moves (every >= 1) first");
    TSU_REQUIRE(ctx, P->have_T, "pt2d_cluster_move: call tsu_pt2d_set_temperatures first");
    TSU_REQUIRE(ctx, P->have_init, "pt2d_cluster_move: call tsu_pt2d_init first");
    TSU_REQUIRE(ctx, P->icm_passes < 0xFFFFFFFFu, "pt2d_cluster_move: cluster-pass counter overflow");
    const int rc = ising2d_check_err(P->lat[0]);  // a cap that expired in an earlier pass
    return rc != TSU_OK ? rc : pt2d_icm_enqueue(P);
}

int tsu_pt2d_cluster_stats(tsu_pt2d* P, int64_t* passes, int64_t* clusters, int64_t* flipped, uint64_t* pass_count, uint64_t* n_launches) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    const size_t row = (size_t)P->R * sizeof(int64_t);
    int64_t* const out[3] = {passes, clusters, flipped};
    for (int k = 0; k < 3; ++k) {
        if (!out[k]) continue;
        if (P->d_icm_stats)
            TSU_HIP_TRY(ctx, hipMemcpyAsync(out[k], P->d_icm_stats + (size_t)k * P->R, row, hipMemcpyDeviceToHost, ctx->stream));
        else
            memset(out[k], 0, row);
    }
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (pass_count) *pass_count = P->icm_passes;
    if (n_launches) *n_launches = P->icm_launches;
    return ising2d_check_err(P->lat[0]);
}

}  // extern "C"

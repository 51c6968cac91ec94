// sw_host.h -- the host side of a Swendsen-Wang call, written once for K6 (ising2d_cluster.hip), K8 (ising3d_cluster.hip) and K10
// (potts_host.h: one traits template, PottsSw, for its 2-D and 3-D handles): the counter checks, the one-workgroup launch with its
// batch upload, the loop of the multi-tile route and the batch entry point's loop.
// A traits struct Tr per handle type supplies what differs:
//   Lattice, Bonds, Model      the handle (with ctx, h_err and a tsu_sw_scratch sw), the bond policy of sw_dev.h, the model
//                              parameters of one call (K6: J and T; K8: T)
//   who, refuse_twice          the prefix of every message; whether a batch refuses a lattice listed twice
//   small, local, merge, resolve   the kernels; small_measured: the one-workgroup kernel that also writes cluster-size records
//   check_model(L, m)          the checks only this dimension has, made ahead of the counter checks
//   check_err(L)               report (and clear) a flag an earlier call's kernel left
//   geom(L), spins(L), bonds(L, m)   extents, pitch and wraps (DIM = 2: depth 1, pz 0); row 0; the policy's values
//   tile_forced()              the environment switch of the tile shape is set: every lattice on the multi-tile route
//   tile(L, g)                 the tile shape into g, checked
//   local_threads(g)           lanes of a tile's workgroup
//   grow_labels(L, bytes)      the labels buffer, with this dimension's message when memory runs out
#pragma once
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ising2d.h"
#include "sw_dev.h"

namespace {

constexpr int kSwSmallSites = 16384;  // one-workgroup route: at most this many sites (80 KB of LDS, 144 KB measured); also the largest tile

template <int DIM>
long long sw_sites(const SwGeom& g) {
    return (long long)(DIM == 3 ? g.depth : 1) * g.rows * g.cols;
}

inline int sw_threads(long long work_items) {
    const long long t = (work_items + 63) / 64 * 64;
    return (int)(t < kSwMaxThreads ? t : kSwMaxThreads);
}

// ---------------------------------------------------------------- the tiles of a 3-D lattice (K8, and K10 in 3-D)
// TSU_SW3D_TILE=<tz>x<tr>x<tc> (tests only, read per call): that tile shape, and every lattice on the multi-tile route.
// 1: a shape was read; 0: the switch is not set; -1: it does not parse
inline int sw3d_tile_switch(SwGeom* t) {
    const char* e = getenv("TSU_SW3D_TILE");
    if (!e || !*e) return 0;
    char tail = 0;
    return sscanf(e, "%dx%dx%d%c", &t->tz, &t->tr, &t->tc, &tail) == 3 ? 1 : -1;
}

inline bool sw3d_tile_forced() {
    SwGeom t;
    return sw3d_tile_switch(&t) != 0;
}

// The tile shape into g, checked.  The default: 16 x 32 x 32 (80 KB of LDS, 1024 lanes, two tiles a CU) leaves 1/16 + 1/32 + 1/32 =
// 12.5 % of a site's three bonds' worth on seams (4.2 % of the bonds); 8 x 16 x 32 (20 KB, 256 lanes) leaves 21.9 % (7.3 % of the
// bonds) but gives four times the workgroups.  The large tile is taken once it fills the chip (one tile per CU at least), the small
// one below that (DESIGN.md section 5, K8 cluster steps).
inline int sw3d_tile(tsu_ctx* ctx, int depth, int rows, int cols, SwGeom& g) {
    const int sw = sw3d_tile_switch(&g);
    TSU_REQUIRE(ctx, sw >= 0, "TSU_SW3D_TILE must read <tz>x<tr>x<tc>");
    if (sw == 0) {
        const long long n_big = (long long)((depth + 15) / 16) * ((rows + 31) / 32) * ((cols + 31) / 32);
        const bool big = n_big >= (ctx->cus > 0 ? ctx->cus : 256);
        g.tz = big ? 16 : 8;
        g.tr = big ? 32 : 16;
        g.tc = 32;
    }
    TSU_REQUIRE(ctx, g.tz >= 1 && g.tr >= 1 && g.tc >= 2 && (g.tc & 1) == 0 && g.tz <= kSwSmallSites && g.tr <= kSwSmallSites &&
                         g.tc <= kSwSmallSites && (long long)g.tz * g.tr * g.tc <= kSwSmallSites,
                "TSU_SW3D_TILE: a tile needs positive extents, an even width and at most %d sites (got %d x %d x %d)", kSwSmallSites, g.tz,
                g.tr, g.tc);
    return TSU_OK;
}

template <class Tr>
bool sw_small_route(const typename Tr::Lattice* L) {
    return !Tr::tile_forced() && sw_sites<Tr::DIM>(Tr::geom(L)) <= kSwSmallSites;
}

template <class Tr>
SwItem<typename Tr::Bonds> sw_make_item(const typename Tr::Lattice* L, const typename Tr::Model& m, uint64_t seed, uint32_t step0,
                                        uint32_t replica) {
    SwItem<typename Tr::Bonds> it;
    it.s = Tr::spins(L);
    it.b = Tr::bonds(L, m);
    it.k.k0 = (uint32_t)seed;
    it.k.k1 = (uint32_t)(seed >> 32);
    it.k.tag_bond = TSU_TAG_SW_BOND | (replica << 8);
    it.k.tag_layer = TSU_TAG_SW_LAYER | (replica << 8);
    it.k.tag_flip = TSU_TAG_SW_FLIP | (replica << 8);
    it.k.tag_ghost = TSU_TAG_SW_GHOST | (replica << 8);
    it.k.t = step0;
    return it;
}

template <class Tr>
int sw_check_call(typename Tr::Lattice* L, const typename Tr::Model& m, int n_steps, uint32_t step0, uint32_t replica) {
    tsu_ctx* ctx = L->ctx;
    const int rc = Tr::check_model(L, m);
    if (rc != TSU_OK) return rc;
    TSU_REQUIRE(ctx, n_steps >= 0, "%s: n_steps must be >= 0", Tr::who);
    TSU_REQUIRE(ctx, (uint64_t)step0 + (uint64_t)n_steps <= (1ull << 32), "%s: step counter overflow", Tr::who);
    TSU_REQUIRE(ctx, replica < TSU_REPLICA_LIMIT, "%s: replica id %u is not below 2^24", Tr::who, (unsigned)replica);
    return Tr::check_err(L);  // a cap that expired in an earlier call
}

// the record buffer of a measured call: n_steps rows, zeroed on the stream (a step whose cap expired leaves its row so)
template <class Tr>
int sw_prepare_record(typename Tr::Lattice* L, int n_steps) {
    tsu_ctx* ctx = L->ctx;
    const size_t bytes = (size_t)n_steps * TSU_CLUSTER_RECORD_WORDS * sizeof(int64_t);
    TSU_HIP_TRY(ctx, ising2d_grow(L->sw.d_rec, L->sw.rec_cap, bytes));
    TSU_HIP_TRY(ctx, hipMemsetAsync(L->sw.d_rec, 0, bytes, ctx->stream));
    L->sw.rec_rows = n_steps;
    return TSU_OK;
}

// n lattices of one shape and boundary, one workgroup each, all steps in one launch.  All of them agree on the measuring switch; on:
// the measured instantiation (9 B of LDS a site instead of 5), every workgroup writing its lattice's rows
template <class Tr>
int sw_run_small(typename Tr::Lattice* const* lats, int n, const SwItem<typename Tr::Bonds>* items, int n_steps) {
    using Item = SwItem<typename Tr::Bonds>;
    typename Tr::Lattice* L0 = lats[0];
    tsu_ctx* ctx = L0->ctx;
    int* d_err = nullptr;
    int rc = tsu_err_flag(ctx, L0->h_err, &d_err);
    if (rc != TSU_OK) return rc;
    const bool measure = L0->sw.measure != 0;
    const SwGeom g = Tr::geom(L0);
    const size_t lds = (size_t)sw_sites<Tr::DIM>(g) * (measure ? 9 : 5);
    TSU_HIP_TRY(ctx, tsu_func_allow_lds(ctx, measure ? (const void*)Tr::small_measured : (const void*)Tr::small, (int)lds));
    SwRecOut rec = {nullptr, nullptr};
    if (measure) {
        for (int i = 0; i < n; ++i)
            if ((rc = sw_prepare_record<Tr>(lats[i], n_steps)) != TSU_OK) return rc;
        rec.rows_one = (long long*)L0->sw.d_rec;
    }
    const Item* d_items = nullptr;
    if (n > 1) {
        const size_t bytes = (size_t)n * sizeof(Item);
        TSU_HIP_TRY(ctx, ising2d_grow(L0->sw.d_batch, L0->sw.batch_cap, bytes));
        std::vector<long long*> rows_of;
        if (measure) {
            for (int i = 0; i < n; ++i) rows_of.push_back((long long*)lats[i]->sw.d_rec);
            TSU_HIP_TRY(ctx, ising2d_grow(L0->sw.d_recs, L0->sw.recs_cap, (size_t)n * sizeof(long long*)));
            TSU_HIP_TRY(ctx, hipMemcpyAsync(L0->sw.d_recs, rows_of.data(), (size_t)n * sizeof(long long*), hipMemcpyHostToDevice, ctx->stream));
            rec.rows_of = (long long* const*)L0->sw.d_recs;
        }
        // the host arrays die with this call: wait for the copies (a few KB); the launch itself stays asynchronous
        TSU_HIP_TRY(ctx, hipMemcpyAsync(L0->sw.d_batch, items, bytes, hipMemcpyHostToDevice, ctx->stream));
        TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        d_items = (const Item*)L0->sw.d_batch;
    }
    const int threads = sw_threads(sw_sites<Tr::DIM>(g) / g.cols * ((g.cols + 1) / 2));
    if (measure)
        hipLaunchKernelGGL(Tr::small_measured, dim3((unsigned)n), dim3((unsigned)threads), lds, ctx->stream, d_items, items[0], g, n_steps, d_err, rec);
    else
        hipLaunchKernelGGL(Tr::small, dim3((unsigned)n), dim3((unsigned)threads), lds, ctx->stream, d_items, items[0], g, n_steps, d_err);
    TSU_HIP_TRY(ctx, hipGetLastError());
    for (int i = 0; i < n; ++i) lats[i]->sw.launches += 1;
    return TSU_OK;
}

// local, merge (when the lattice has a seam or a wrap) and resolve, once per step
template <class Tr>
int sw_run_tiles(typename Tr::Lattice* L, const SwItem<typename Tr::Bonds>& it, int n_steps) {
    tsu_ctx* ctx = L->ctx;
    SwParams<typename Tr::Bonds> p;
    SwGeom& g = p.g;
    g = Tr::geom(L);
    int rc = Tr::tile(L, g);
    if (rc != TSU_OK) return rc;
    g.nz = (g.depth + g.tz - 1) / g.tz;
    g.nr = (g.rows + g.tr - 1) / g.tr;
    g.nc = (g.cols + g.tc - 1) / g.tc;
    rc = Tr::grow_labels(L, (size_t)sw_sites<Tr::DIM>(g) * sizeof(int32_t));
    if (rc != TSU_OK) return rc;
    p.s = it.s;
    p.labels = L->sw.d_labels;
    p.b = it.b;
    p.k = it.k;
    rc = tsu_err_flag(ctx, L->h_err, &p.err);
    if (rc != TSU_OK) return rc;
    const long long n_tiles = (long long)g.nz * g.nr * g.nc;
    TSU_REQUIRE(ctx, n_tiles < (1ll << 31), "%s: %lld tiles exceed the grid", Tr::who, n_tiles);
    const long long merge_lanes = sw_seam_lanes<Tr::DIM>(g);
    const size_t lds = (size_t)g.tz * g.tr * g.tc * 5;
    TSU_HIP_TRY(ctx, tsu_func_allow_lds(ctx, (const void*)Tr::local, (int)lds));
    const unsigned local_threads = (unsigned)Tr::local_threads(g);
    const int quads = (g.cols + 3) / 4;
    const unsigned resolve_blocks = (unsigned)((sw_sites<Tr::DIM>(g) / g.cols * quads + 255) / 256);
    // measuring (tsu_hip_cluster_measure.h): sw_meas_count between the local and the merge pass, sw_meas_fold (where there is a
    // merge pass) and sw_meas_row after it; the unmeasured kernels and their launches are the same either way
    const bool measure = L->sw.measure != 0;
    SwMeasParams m = {};
    unsigned meas_blocks = 0;
    const size_t meas_lds = (size_t)g.tz * g.tr * g.tc * sizeof(unsigned);
    if (measure) {
        const long long sites = sw_sites<Tr::DIM>(g);
        if ((rc = sw_prepare_record<Tr>(L, n_steps)) != TSU_OK) return rc;
        TSU_HIP_TRY(ctx, ising2d_grow(L->sw.d_acc, L->sw.acc_cap, (size_t)(sites + 2) * sizeof(unsigned long long)));
        TSU_HIP_TRY(ctx, hipMemsetAsync(L->sw.d_acc + sites, 0, 2 * sizeof(unsigned long long), ctx->stream));
        TSU_HIP_TRY(ctx, tsu_func_allow_lds(ctx, (const void*)sw_meas_count<Tr::DIM>, (int)meas_lds));
        m.s = p.s;
        m.labels = p.labels;
        m.acc = L->sw.d_acc;
        m.sites = sites;
        m.g = g;
        m.err = p.err;
        meas_blocks = (unsigned)((sites + 255) / 256 < 2048 ? (sites + 255) / 256 : 2048);
    }
    for (int s = 0; s < n_steps; ++s) {
        p.k.t = it.k.t + (uint32_t)s;
        if (measure) m.row = (unsigned long long*)L->sw.d_rec + (size_t)s * TSU_CLUSTER_RECORD_WORDS;
        hipLaunchKernelGGL(Tr::local, dim3((unsigned)n_tiles), dim3(local_threads), lds, ctx->stream, p);
        if (measure) hipLaunchKernelGGL(sw_meas_count<Tr::DIM>, dim3((unsigned)n_tiles), dim3(256), meas_lds, ctx->stream, m);
        if (merge_lanes > 0) hipLaunchKernelGGL(Tr::merge, dim3((unsigned)((merge_lanes + 255) / 256)), dim3(256), 0, ctx->stream, p);
        if (measure && merge_lanes > 0) hipLaunchKernelGGL(sw_meas_fold<Tr::DIM>, dim3(meas_blocks), dim3(256), 0, ctx->stream, m);
        if (measure) hipLaunchKernelGGL(sw_meas_row<Tr::DIM>, dim3(meas_blocks), dim3(256), 0, ctx->stream, m);
        hipLaunchKernelGGL(Tr::resolve, dim3(resolve_blocks), dim3(256), 0, ctx->stream, p, quads);
        L->sw.launches += (merge_lanes > 0 ? 3 : 2) + (measure ? (merge_lanes > 0 ? 3 : 2) : 0);
    }
    TSU_HIP_TRY(ctx, hipGetLastError());
    return TSU_OK;
}

template <class Tr>
int sw_sweep(typename Tr::Lattice* L, const typename Tr::Model& m, int n_steps, uint64_t seed, uint32_t step0, uint32_t replica) {
    if (!L) return TSU_E_INVALID;
    const int rc = sw_check_call<Tr>(L, m, n_steps, step0, replica);
    if (rc != TSU_OK || n_steps == 0) return rc;
    const auto it = sw_make_item<Tr>(L, m, seed, step0, replica);
    return sw_small_route<Tr>(L) ? sw_run_small<Tr>(&L, 1, &it, n_steps) : sw_run_tiles<Tr>(L, it, n_steps);
}

// the measuring switch of a handle, and the rows of its most recent measured call (tsu_hip_cluster_measure.h)
template <class Tr>
int sw_measure(typename Tr::Lattice* L, int on) {
    if (!L) return TSU_E_INVALID;
    L->sw.measure = on != 0;  // nothing is allocated before the next cluster call, nothing freed before the handle goes
    return TSU_OK;
}

template <class Tr>
int sw_record(typename Tr::Lattice* L, int64_t* rows, int max_rows, int* n_rows) {
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, n_rows && max_rows >= 0 && (rows || max_rows == 0), "%s_record: n_rows is NULL, max_rows negative or rows NULL", Tr::who);
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const int rc = Tr::check_err(L);
    if (rc != TSU_OK) return rc;
    *n_rows = L->sw.rec_rows;
    const int n = L->sw.rec_rows < max_rows ? L->sw.rec_rows : max_rows;
    if (n > 0) TSU_HIP_TRY(ctx, hipMemcpy(rows, L->sw.d_rec, (size_t)n * TSU_CLUSTER_RECORD_WORDS * sizeof(int64_t), hipMemcpyDeviceToHost));
    return TSU_OK;
}

// every lattice checked first; one launch if all of them take the one-workgroup route with one shape and boundary and agree on the
// measuring switch, else one by one.
// model_of(i): the Model of lattice i
template <class Tr, class ModelOf>
int sw_sweep_batch(typename Tr::Lattice* const* lats, int n_lats, int n_steps, ModelOf model_of, const uint64_t* seeds,
                   const uint32_t* step0s, const uint32_t* replicas) {
    tsu_ctx* ctx = lats[0]->ctx;
    const SwGeom a = Tr::geom(lats[0]);
    bool one_launch = true;
    for (int i = 0; i < n_lats; ++i) {
        typename Tr::Lattice* L = lats[i];
        TSU_REQUIRE(ctx, L && L->ctx == ctx, "%s_sweep_batch: lattice %d is NULL or belongs to another context", Tr::who, i);
        if (Tr::refuse_twice)
            for (int k = 0; k < i; ++k) TSU_REQUIRE(ctx, lats[k] != L, "%s_sweep_batch: lattice %d appears twice", Tr::who, i);
        const int rc = sw_check_call<Tr>(L, model_of(i), n_steps, step0s[i], replicas[i]);
        if (rc != TSU_OK) return rc;
        const SwGeom g = Tr::geom(L);
        one_launch = one_launch && sw_small_route<Tr>(L) && g.depth == a.depth && g.rows == a.rows && g.cols == a.cols && g.pz == a.pz &&
                     g.pr == a.pr && g.pc == a.pc && (L->sw.measure != 0) == (lats[0]->sw.measure != 0);
    }
    if (n_steps == 0) return TSU_OK;
    if (one_launch) {
        std::vector<SwItem<typename Tr::Bonds>> items((size_t)n_lats);
        for (int i = 0; i < n_lats; ++i) items[(size_t)i] = sw_make_item<Tr>(lats[i], model_of(i), seeds[i], step0s[i], replicas[i]);
        return sw_run_small<Tr>(lats, n_lats, items.data(), n_steps);
    }
    for (int i = 0; i < n_lats; ++i) {
        const int rc = sw_sweep<Tr>(lats[i], model_of(i), n_steps, seeds[i], step0s[i], replicas[i]);
        if (rc != TSU_OK) return rc;
    }
    return TSU_OK;
}

}  // namespace

// potts_host.h -- the host side of K10, the q-state Potts lattice, written once for the 2-D handle (potts2d.hip, tsu_hip_potts.h)
// and the 3-D one (potts3d.hip, tsu_hip_potts3d.h): the handle's fields, the heat-bath and measuring launches, the traits of the
// Swendsen-Wang steps for sw_host.h, and the body of every entry point as a template over the handle type L.  tsu_potts2d and
// tsu_potts3d stay distinct types (PottsHandle<2> and PottsHandle<3> by inheritance); their extern "C" functions forward here.
// The kernels are potts_kern_dev.h's, instantiated at L::DIM, so a 2-D handle launches nothing that carries a z term.
#pragma once
#include <math.h>
#include <stdlib.h>

#include "potts_kern_dev.h"
#include "sw_host.h"

static_assert(TSU_POTTS_ROUTE_SMALL == TSU_POTTS3D_ROUTE_SMALL && TSU_POTTS_ROUTE_SWEEP == TSU_POTTS3D_ROUTE_SWEEP &&
                  TSU_POTTS_ROUTE_SW_SMALL == TSU_POTTS3D_ROUTE_SW_SMALL && TSU_POTTS_ROUTE_SW_TILES == TSU_POTTS3D_ROUTE_SW_TILES,
              "one route numbering serves both handles");

template <int D>
struct PottsHandle {
    static constexpr int DIM = D;
    static constexpr const char* name = D == 2 ? "potts2d" : "potts3d";  // the prefix of every message
    tsu_ctx* ctx;
    PottsGeom g;  // DIM = 2: depth 1, pz 0
    int q;
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

constexpr int kPottsTile = 64;  // the edge of a 2-D tile

inline uint64_t potts_threshold(double J, double T) {
    const double p = -expm1(-J / T);
    return (uint64_t)floor(p * 4294967296.0);
}

template <class L>
long long potts_sites(const L* H) {
    return (long long)H->g.depth * H->g.rows * H->g.cols;
}

template <class L>
int potts_check_err(L* H) {
    if (H->h_err && *H->h_err) {
        *H->h_err = 0;
        return tsu_fail(H->ctx, TSU_E_HIP, "%s: a cluster kernel's union / find loop hit its iteration cap; results invalid", L::name);
    }
    return TSU_OK;
}

// ---------------------------------------------------------------- the Swendsen-Wang steps' traits (sw_host.h)
inline int potts_tile_switch() {
    const char* e = getenv("TSU_SW_TILE");
    return e ? atoi(e) : 0;
}

template <class L>
struct PottsSw {
    static constexpr int DIM = L::DIM;
    using Lattice = L;
    using Bonds = PottsBonds;
    struct Model {
        double T;
    };
    static constexpr const char* who = DIM == 2 ? "potts2d_cluster" : "potts3d_cluster";
    [[maybe_unused]] static constexpr bool refuse_twice = false;  // no batch entry point
    static constexpr auto small = k10_sw_small<DIM>;
    static constexpr auto small_measured = k10_sw_small<DIM, SwRecOut>;  // never launched: sw.measure stays 0
    static constexpr auto local = k10_sw_local<DIM>;
    static constexpr auto merge = k10_sw_merge<DIM>;
    static constexpr auto resolve = k10_sw_resolve<DIM>;

    static int check_model(L* H, const Model& m) {
        tsu_ctx* ctx = H->ctx;
        TSU_REQUIRE(ctx, isfinite(m.T) && m.T > 0.0, "Temperature must be positive");
        if (!(H->J > 0.0)) return tsu_fail(ctx, TSU_E_UNSUPPORTED, "%s: Swendsen-Wang steps need J > 0 (heat-bath sweeps take J <= 0)", who);
        for (int c = 0; c < H->q; ++c)
            if (H->h[c] != 0.0) return tsu_fail(ctx, TSU_E_UNSUPPORTED, "%s: Swendsen-Wang steps need a zero field", who);
        return TSU_OK;
    }
    static int check_err(L* H) { return potts_check_err(H); }
    static SwGeom geom(const L* H) {
        SwGeom g = {};
        g.pitch = (long long)H->g.cols;
        g.depth = H->g.depth;
        g.rows = H->g.rows;
        g.cols = H->g.cols;
        g.pz = H->g.pz;
        g.pr = H->g.pr;
        g.pc = H->g.pc;
        return g;
    }
    static int8_t* spins(const L* H) { return H->d_s; }
    static Bonds bonds(const L* H, const Model& m) { return Bonds{potts_threshold(H->J, m.T), H->q}; }
    static bool tile_forced() {
        if constexpr (DIM == 2) return potts_tile_switch() != 0;
        else return sw3d_tile_forced();
    }
    static int tile(L* H, SwGeom& g) {
        if constexpr (DIM == 2) {
            int edge = potts_tile_switch();
            if (edge <= 0) edge = kPottsTile;
            TSU_REQUIRE(H->ctx, edge >= 2 && edge <= 64 && (edge & 1) == 0, "TSU_SW_TILE must be an even edge in [2, 64] (got %d)", edge);
            g.tz = 1;
            g.tr = g.tc = edge;
            return TSU_OK;
        } else {
            return sw3d_tile(H->ctx, H->g.depth, H->g.rows, H->g.cols, g);
        }
    }
    static int local_threads(const SwGeom& g) {
        if constexpr (DIM == 2) return kPottsLocalThreads;
        else return sw_threads((g.tz * g.tr * g.tc + 15) / 16);
    }
    static int grow_labels(L* H, size_t bytes) {
        if constexpr (DIM == 2) {
            TSU_HIP_TRY(H->ctx, ising2d_grow(H->sw.d_labels, H->sw.labels_cap, bytes));
            return TSU_OK;
        } else {
            const hipError_t e = ising2d_grow(H->sw.d_labels, H->sw.labels_cap, bytes);
            if (e == hipSuccess) return TSU_OK;
            (void)hipGetLastError();
            return tsu_fail(H->ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "potts3d_cluster: the labels buffer: %s (%zu bytes)",
                            hipGetErrorString(e), bytes);
        }
    }
};

// ---------------------------------------------------------------- the heat bath and the observables
inline bool potts_small_switch_off() {  // TSU_POTTS_SMALL=0 (tests, read per call): every lattice on k10_sweep
    const char* e = getenv("TSU_POTTS_SMALL");
    return e && atoi(e) == 0;
}

template <class L>
bool potts_hb_small_route(const L* H) {
    return !potts_small_switch_off() && potts_sites(H) <= kPottsSmallSites;
}

template <class L>
int potts_hb_check(L* H, double T, int n_sweeps, uint32_t replica, PottsTabN<2 * L::DIM>* tab) {
    tsu_ctx* ctx = H->ctx;
    const char* why = potts_tables(H->q, H->J, H->h, T, tab);
    TSU_REQUIRE(ctx, !why, "%s_sweep: %s", L::name, why);
    TSU_REQUIRE(ctx, n_sweeps >= 0, "%s_sweep: n_sweeps must be >= 0", L::name);
    TSU_REQUIRE(ctx, replica < TSU_REPLICA_LIMIT, "%s_sweep: replica id %u is not below 2^24", L::name, (unsigned)replica);
    return TSU_OK;
}

template <class L>
int potts_hb_sweep(L* H, const PottsTabN<2 * L::DIM>& tab, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica) {
    constexpr int DIM = L::DIM;
    tsu_ctx* ctx = H->ctx;
    if (n_sweeps == 0) return TSU_OK;
    PottsSweep<DIM> p;
    p.s = H->d_s;
    p.g = H->g;
    p.k = PottsKeys{(uint32_t)seed, (uint32_t)(seed >> 32), TSU_TAG_ISING_HI | (replica << 8), TSU_TAG_ISING_LO | (replica << 8)};
    p.t = tab;
    const long long lanes = (long long)H->g.depth * H->g.rows * ((H->g.cols + 15) >> 4);
    if (potts_hb_small_route(H)) {
        p.hs = sweep0;
        hipLaunchKernelGGL(k10_small<DIM>, dim3(1), dim3((unsigned)sw_threads(lanes)), 0, ctx->stream, p, n_sweeps);
        H->launches += 1;
    } else {
        const dim3 grid((unsigned)((lanes + 255) / 256));
        for (int k = 0; k < n_sweeps; ++k)
            for (uint32_t colour = 0; colour < 2; ++colour) {
                p.hs = 2u * (sweep0 + (uint32_t)k) + colour;  // 32-bit words: the header says so
                if ((H->g.cols & 15) == 0) hipLaunchKernelGGL((k10_sweep<DIM, true>), grid, dim3(256), 0, ctx->stream, p);
                else hipLaunchKernelGGL((k10_sweep<DIM, false>), grid, dim3(256), 0, ctx->stream, p);
                H->launches += 1;
            }
    }
    TSU_HIP_TRY(ctx, hipGetLastError());
    return TSU_OK;
}

template <class L>
int potts_measure_into(L* H, long long* d_row) {
    tsu_ctx* ctx = H->ctx;
    TSU_HIP_TRY(ctx, hipMemsetAsync(d_row, 0, TSU_POTTS_RECORD_WORDS * sizeof(long long), ctx->stream));
    PottsMeasure m = {H->d_s, H->g, H->q, (unsigned long long*)d_row};
    const long long want = (potts_sites(H) + 255) / 256;
    hipLaunchKernelGGL(k10_measure<L::DIM>, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(256), 0, ctx->stream, m);
    TSU_HIP_TRY(ctx, hipGetLastError());
    H->launches += 1;
    return TSU_OK;
}

// ---------------------------------------------------------------- the entry points' bodies
// tables: E[0 .. NB] then F[0 .. 7], NB = 4 or 6
template <int NB>
int potts_check_model(int q, double J, const double* h, double T, double* tables) {
    PottsTabN<NB> t;
    if (potts_tables(q, J, h, T, &t)) return TSU_E_INVALID;
    if (tables) {
        for (int n = 0; n <= NB; ++n) tables[n] = t.E[n];
        for (int c = 0; c < TSU_POTTS_MAX_Q; ++c) tables[NB + 1 + c] = t.F[c];
    }
    return TSU_OK;
}

// the 2-D entry point passes depth 1 and pz 0, so that each axis is checked as the 3-D one checks it
template <class L>
int potts_create(tsu_ctx* ctx, int depth, int rows, int cols, int q, int pz, int pr, int pc, L** out) {
    TSU_ENTER(ctx);
    if (!ctx || !out) return TSU_E_INVALID;
    TSU_REQUIRE(ctx, q >= 2 && q <= TSU_POTTS_MAX_Q, "%s_create: q must be in 2 .. 8 (got %d)", L::name, q);
    TSU_REQUIRE(ctx, depth >= 1 && rows >= 1 && cols >= 1, "%s_create: %s must be >= 1", L::name,
                L::DIM == 2 ? "rows and cols" : "depth, rows and cols");
    TSU_REQUIRE(ctx, (long long)depth * rows < (1ll << 31) && (long long)depth * rows * cols < (1ll << 31),
                "%s_create: %lld x %d sites exceed 32-bit labels", L::name, (long long)depth * rows, cols);
    TSU_REQUIRE(ctx, (!pz || (depth & 1) == 0) && (!pr || (rows & 1) == 0) && (!pc || (cols & 1) == 0),
                "%s_create: a periodic axis needs an even length", L::name);
    L* H = new L();
    H->ctx = ctx;
    H->g = PottsGeom{depth, pz != 0, pc != 0, rows, cols, pr != 0};
    H->q = q;
    H->J = 1.0;
    const size_t n = (size_t)potts_sites(H);
    hipError_t e = hipMalloc((void**)&H->d_s, n);
    if (e == hipSuccess) e = hipMalloc((void**)&H->d_obs, TSU_POTTS_RECORD_WORDS * sizeof(long long));
    if (e == hipSuccess) e = hipMemsetAsync(H->d_s, 0, n, ctx->stream);
    if (e != hipSuccess) {
        if (H->d_s) (void)hipFree(H->d_s);
        if (H->d_obs) (void)hipFree(H->d_obs);
        delete H;
        return tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "%s_create: %s", L::name, hipGetErrorString(e));
    }
    *out = H;
    return TSU_OK;
}

template <class L>
int potts_destroy(L* H) {
    TSU_ENTER(H ? H->ctx : nullptr);
    if (!H) return TSU_E_INVALID;
    (void)hipStreamSynchronize(H->ctx->stream);
    (void)hipFree(H->d_s);
    (void)hipFree(H->d_obs);
    if (H->d_rec) (void)hipFree(H->d_rec);
    if (H->h_err) (void)hipHostFree(H->h_err);
    tsu_sw_scratch_free(H->sw);
    delete H;
    return TSU_OK;
}

template <class L>
int potts_set_model(L* H, double J, const double* h) {
    TSU_ENTER(H ? H->ctx : nullptr);
    if (!H) return TSU_E_INVALID;
    TSU_REQUIRE(H->ctx, isfinite(J), "%s_set_model: J must be finite", L::name);
    for (int c = 0; h && c < H->q; ++c) TSU_REQUIRE(H->ctx, isfinite(h[c]), "%s_set_model: h must be finite", L::name);
    H->J = J;  // the bound on (NB |J| + max h - min h) / T is checked with every sweep's temperature
    for (int c = 0; c < TSU_POTTS_MAX_Q; ++c) H->h[c] = (h && c < H->q) ? h[c] : 0.0;
    return TSU_OK;
}

template <class L>
int potts_set_spins(L* H, const int8_t* colours) {
    TSU_ENTER(H ? H->ctx : nullptr);
    if (!H) return TSU_E_INVALID;
    tsu_ctx* ctx = H->ctx;
    TSU_REQUIRE(ctx, colours, "%s_set_spins: colours is NULL", L::name);
    const size_t n = (size_t)potts_sites(H);
    for (size_t i = 0; i < n; ++i)
        TSU_REQUIRE(ctx, colours[i] >= 0 && colours[i] < H->q, "%s_set_spins: colour %d at site %zu is outside 0 .. %d", L::name, (int)colours[i], i,
                    H->q - 1);
    TSU_HIP_TRY(ctx, hipMemcpyAsync(H->d_s, colours, n, hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

template <class L>
int potts_get_spins(L* H, int8_t* colours) {
    TSU_ENTER(H ? H->ctx : nullptr);
    if (!H) return TSU_E_INVALID;
    tsu_ctx* ctx = H->ctx;
    TSU_REQUIRE(ctx, colours, "%s_get_spins: colours is NULL", L::name);
    TSU_HIP_TRY(ctx, hipMemcpyAsync(colours, H->d_s, (size_t)potts_sites(H), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return potts_check_err(H);
}

template <class L>
int potts_fill(L* H, int colour) {
    TSU_ENTER(H ? H->ctx : nullptr);
    if (!H) return TSU_E_INVALID;
    TSU_REQUIRE(H->ctx, colour >= 0 && colour < H->q, "%s_fill: colour %d is outside 0 .. %d", L::name, colour, H->q - 1);
    TSU_HIP_TRY(H->ctx, hipMemsetAsync(H->d_s, colour, (size_t)potts_sites(H), H->ctx->stream));
    return TSU_OK;
}

template <class L>
int potts_sweep(L* H, double T, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica) {
    TSU_ENTER(H ? H->ctx : nullptr);
    if (!H) return TSU_E_INVALID;
    PottsTabN<2 * L::DIM> tab;
    const int rc = potts_hb_check(H, T, n_sweeps, replica, &tab);
    if (rc != TSU_OK) return rc;
    return potts_hb_sweep(H, tab, n_sweeps, seed, sweep0, replica);
}

template <class L>
int potts_cluster_sweep(L* H, double T, int n_steps, uint64_t seed, uint32_t step0, uint32_t replica) {
    TSU_ENTER(H ? H->ctx : nullptr);
    return sw_sweep<PottsSw<L>>(H, {T}, n_steps, seed, step0, replica);
}

template <class L>
int potts_route(L* H, int algorithm, int* route) {
    TSU_ENTER(H ? H->ctx : nullptr);
    if (!H || !route) return TSU_E_INVALID;
    TSU_REQUIRE(H->ctx, algorithm == TSU_POTTS_HEAT_BATH || algorithm == TSU_POTTS_SWENDSEN_WANG, "%s_route: unknown algorithm %d", L::name,
                algorithm);
    if (algorithm == TSU_POTTS_HEAT_BATH) *route = potts_hb_small_route(H) ? TSU_POTTS_ROUTE_SMALL : TSU_POTTS_ROUTE_SWEEP;
    else *route = sw_small_route<PottsSw<L>>(H) ? TSU_POTTS_ROUTE_SW_SMALL : TSU_POTTS_ROUTE_SW_TILES;
    return TSU_OK;
}

template <class L>
int potts_measure(L* H, int64_t* row) {
    TSU_ENTER(H ? H->ctx : nullptr);
    if (!H) return TSU_E_INVALID;
    tsu_ctx* ctx = H->ctx;
    TSU_REQUIRE(ctx, row, "%s_measure: row is NULL", L::name);
    const int rc = potts_measure_into(H, H->d_obs);
    if (rc != TSU_OK) return rc;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(row, H->d_obs, TSU_POTTS_RECORD_WORDS * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return potts_check_err(H);
}

template <class L>
int potts_run(L* H, double T, int n_meas, int sweeps_between, int algorithm, uint64_t seed, uint32_t counter0, uint32_t replica) {
    using Sw = PottsSw<L>;
    TSU_ENTER(H ? H->ctx : nullptr);
    if (!H) return TSU_E_INVALID;
    tsu_ctx* ctx = H->ctx;
    const bool hb = algorithm == TSU_POTTS_HEAT_BATH;
    TSU_REQUIRE(ctx, hb || algorithm == TSU_POTTS_SWENDSEN_WANG, "%s_run: unknown algorithm %d", L::name, algorithm);
    TSU_REQUIRE(ctx, n_meas >= 0 && sweeps_between >= 0, "%s_run: n_meas and sweeps_between must be >= 0", L::name);
    const long long total = (long long)n_meas * sweeps_between;
    TSU_REQUIRE(ctx, total <= (1ll << 31), "%s_run: %lld updates exceed one call", L::name, total);
    PottsTabN<2 * L::DIM> tab;
    int rc = hb ? potts_hb_check(H, T, sweeps_between, replica, &tab) : sw_check_call<Sw>(H, {T}, 0, counter0, replica);
    if (rc != TSU_OK) return rc;
    TSU_REQUIRE(ctx, hb || (uint64_t)counter0 + (uint64_t)total <= (1ull << 32), "%s_run: step counter overflow", L::name);
    const size_t bytes = (size_t)n_meas * TSU_POTTS_RECORD_WORDS * sizeof(long long);
    TSU_HIP_TRY(ctx, ising2d_grow(H->d_rec, H->rec_cap, bytes ? bytes : sizeof(long long)));
    H->rec_rows = 0;
    for (int k = 0; k < n_meas; ++k) {
        const uint32_t c0 = counter0 + (uint32_t)((long long)k * sweeps_between);
        rc = hb ? potts_hb_sweep(H, tab, sweeps_between, seed, c0, replica) : sw_sweep<Sw>(H, {T}, sweeps_between, seed, c0, replica);
        if (rc == TSU_OK) rc = potts_measure_into(H, H->d_rec + (size_t)k * TSU_POTTS_RECORD_WORDS);
        if (rc != TSU_OK) return rc;
        H->rec_rows = k + 1;
    }
    return TSU_OK;
}

template <class L>
int potts_record(L* H, int64_t* rows, int max_rows, int* n_rows) {
    TSU_ENTER(H ? H->ctx : nullptr);
    if (!H) return TSU_E_INVALID;
    tsu_ctx* ctx = H->ctx;
    TSU_REQUIRE(ctx, n_rows && max_rows >= 0 && (rows || max_rows == 0), "%s_record: n_rows is NULL, max_rows negative or rows NULL", L::name);
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const int rc = potts_check_err(H);
    if (rc != TSU_OK) return rc;
    *n_rows = H->rec_rows;
    const int n = H->rec_rows < max_rows ? H->rec_rows : max_rows;
    if (n > 0) TSU_HIP_TRY(ctx, hipMemcpy(rows, H->d_rec, (size_t)n * TSU_POTTS_RECORD_WORDS * sizeof(int64_t), hipMemcpyDeviceToHost));
    return TSU_OK;
}

template <class L>
int potts_launch_count(L* H, uint64_t* n) {
    TSU_ENTER(H ? H->ctx : nullptr);
    if (!H || !n) return TSU_E_INVALID;
    *n = H->launches + H->sw.launches;
    return TSU_OK;
}

}  // namespace

// potts_disorder.hip -- K12: q-state Potts lattices with per-bond couplings and per-site colour fields (gfx950), the host side and the
// C ABI of include/tsu_hip_potts_disorder.h; the contracts are DESIGN.md section 3.  The kernels are potts_disorder_kern_dev.h's, the
// decision rule potts_disorder_dev.h's (host and device).  One handle serves both dimensions: a lattice with depth 1 and an open z
// axis launches the DIM = 2 instantiations, every other one DIM = 3.  The Swendsen-Wang steps run through sw_host.h on a traits
// struct of their own (PdSw), whose bond policy carries the stored couplings.  K10's files are used as they stand.
#include <math.h>
#include <stdlib.h>

#include "potts_disorder_kern_dev.h"
#include "sw_host.h"

struct tsu_potts_dis {
    tsu_ctx* ctx;
    PottsGeom g;  // 2-D: depth 1, pz 0
    int dim, q;
    int8_t* d_s;   // depth * rows * cols colours, pitch = cols
    float* d_dis;  // J_right, J_down, J_layer (3-D), then the q colour planes of h (when given), one allocation
    PdModel m;     // the planes' addresses, sites and q; T is set per call
    int have_disorder, have_field, sw_ok;
    int* h_err;         // host-mapped flag of the cluster kernels (2: a capped union / find loop expired)
    tsu_sw_scratch sw;  // labels and launches of the cluster steps
    long long* d_obs;   // one measurement row
    long long* d_rec;   // the rows of the most recent run
    size_t rec_cap;
    int rec_rows;
    double* d_part;               // kEnergyBlocks partials of the energy sum
    unsigned long long launches;  // heat-bath and measuring launches
};

namespace {

constexpr int kPdTile = 64;  // the edge of a 2-D tile, as K10's

long long pd_sites(const tsu_potts_dis* H) { return (long long)H->g.depth * H->g.rows * H->g.cols; }

int pd_check_err(tsu_potts_dis* H) {
    if (H->h_err && *H->h_err) {
        *H->h_err = 0;
        return tsu_fail(H->ctx, TSU_E_HIP, "potts_dis: a cluster kernel's union / find loop hit its iteration cap; results invalid");
    }
    return TSU_OK;
}

// ---------------------------------------------------------------- the Swendsen-Wang steps' traits (sw_host.h)
template <int D>
struct PdSw {
    static constexpr int DIM = D;
    using Lattice = tsu_potts_dis;
    using Bonds = PdBonds;
    struct Model {
        double T;
    };
    static constexpr const char* who = "potts_dis_cluster";
    [[maybe_unused]] static constexpr bool refuse_twice = false;  // no batch entry point
    static constexpr auto small = k12_sw_small<DIM>;
    static constexpr auto small_measured = k12_sw_small<DIM, SwRecOut>;  // never launched: sw.measure stays 0
    static constexpr auto local = k12_sw_local<DIM>;
    static constexpr auto merge = k12_sw_merge<DIM>;
    static constexpr auto resolve = k12_sw_resolve<DIM>;

    static int check_model(tsu_potts_dis* H, const Model& m) {
        tsu_ctx* ctx = H->ctx;
        TSU_REQUIRE(ctx, H->have_disorder, "%s: call tsu_potts_dis_set_disorder first", who);
        TSU_REQUIRE(ctx, isfinite(m.T) && m.T > 0.0, "Temperature must be positive");
        if (!H->sw_ok)
            return tsu_fail(ctx, TSU_E_UNSUPPORTED, "%s: Swendsen-Wang steps need every coupling >= 0 and a zero field (heat-bath sweeps take any)",
                            who);
        return TSU_OK;
    }
    static int check_err(tsu_potts_dis* H) { return pd_check_err(H); }
    static SwGeom geom(const tsu_potts_dis* H) {
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
    static int8_t* spins(const tsu_potts_dis* H) { return H->d_s; }
    static Bonds bonds(const tsu_potts_dis* H, const Model& m) { return Bonds{H->m.jr, H->m.jd, H->m.jl, m.T, H->q}; }
    static int tile_switch() {
        const char* e = getenv("TSU_SW_TILE");
        return e ? atoi(e) : 0;
    }
    static bool tile_forced() {
        if constexpr (DIM == 2) return tile_switch() != 0;
        else return sw3d_tile_forced();
    }
    static int tile(tsu_potts_dis* H, SwGeom& g) {
        if constexpr (DIM == 2) {
            int edge = tile_switch();
            if (edge <= 0) edge = kPdTile;
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
    static int grow_labels(tsu_potts_dis* H, size_t bytes) {
        const hipError_t e = ising2d_grow(H->sw.d_labels, H->sw.labels_cap, bytes);
        if (e == hipSuccess) return TSU_OK;
        (void)hipGetLastError();
        return tsu_fail(H->ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "potts_dis_cluster: the labels buffer: %s (%zu bytes)",
                        hipGetErrorString(e), bytes);
    }
};

// ---------------------------------------------------------------- the heat bath and the observables
bool pd_small_switch_off() {  // TSU_POTTS_SMALL=0 (tests, read per call): every lattice on k12_sweep
    const char* e = getenv("TSU_POTTS_SMALL");
    return e && atoi(e) == 0;
}

bool pd_hb_small_route(const tsu_potts_dis* H) { return !pd_small_switch_off() && pd_sites(H) <= kPottsSmallSites; }

int pd_hb_check(tsu_potts_dis* H, double T, int n_sweeps, uint32_t replica) {
    tsu_ctx* ctx = H->ctx;
    TSU_REQUIRE(ctx, H->have_disorder, "potts_dis_sweep: call tsu_potts_dis_set_disorder first");
    TSU_REQUIRE(ctx, isfinite(T) && T > 0.0, "Temperature must be positive");
    TSU_REQUIRE(ctx, n_sweeps >= 0, "potts_dis_sweep: n_sweeps must be >= 0");
    TSU_REQUIRE(ctx, replica < TSU_REPLICA_LIMIT, "potts_dis_sweep: replica id %u is not below 2^24", (unsigned)replica);
    return TSU_OK;
}

template <int DIM, bool HAS_H>
void pd_hb_launch(tsu_potts_dis* H, PdSweep<DIM>& p, int n_sweeps, uint32_t sweep0) {
    hipStream_t st = H->ctx->stream;
    const long long lanes = (long long)H->g.depth * H->g.rows * ((H->g.cols + 15) >> 4);
    if (pd_hb_small_route(H)) {
        p.hs = sweep0;
        hipLaunchKernelGGL((k12_small<DIM, HAS_H>), dim3(1), dim3((unsigned)sw_threads(lanes)), 0, st, p, n_sweeps);
        H->launches += 1;
        return;
    }
    const dim3 grid((unsigned)((lanes + 255) / 256));
    for (int k = 0; k < n_sweeps; ++k)
        for (uint32_t colour = 0; colour < 2; ++colour) {
            p.hs = 2u * (sweep0 + (uint32_t)k) + colour;  // 32-bit words: the header says so
            if ((H->g.cols & 15) == 0) hipLaunchKernelGGL((k12_sweep<DIM, true, HAS_H>), grid, dim3(256), 0, st, p);
            else hipLaunchKernelGGL((k12_sweep<DIM, false, HAS_H>), grid, dim3(256), 0, st, p);
            H->launches += 1;
        }
}

template <int DIM>
int pd_hb_sweep(tsu_potts_dis* H, double T, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica) {
    if (n_sweeps == 0) return TSU_OK;
    PdSweep<DIM> p;
    p.s = H->d_s;
    p.g = H->g;
    p.k = PottsKeys{(uint32_t)seed, (uint32_t)(seed >> 32), TSU_TAG_ISING_HI | (replica << 8), TSU_TAG_ISING_LO | (replica << 8)};
    p.hs = 0;
    p.m = H->m;
    p.m.T = T;
    if (H->have_field) pd_hb_launch<DIM, true>(H, p, n_sweeps, sweep0);
    else pd_hb_launch<DIM, false>(H, p, n_sweeps, sweep0);
    TSU_HIP_TRY(H->ctx, hipGetLastError());
    return TSU_OK;
}

// the grid of a measurement: a function of the shape alone, at most kEnergyBlocks workgroups
unsigned pd_measure_blocks(const tsu_potts_dis* H) { return reduce_blocks(pd_sites(H)); }

// one row of TSU_POTTS_DIS_RECORD_WORDS words at d_row: the integers, then E
int pd_measure_into(tsu_potts_dis* H, long long* d_row) {
    tsu_ctx* ctx = H->ctx;
    TSU_HIP_TRY(ctx, hipMemsetAsync(d_row, 0, TSU_POTTS_DIS_RECORD_WORDS * sizeof(long long), ctx->stream));
    PdMeasure m = {H->d_s, H->g, H->m, (unsigned long long*)d_row, H->d_part};
    m.m.q = H->q;
    const unsigned blocks = pd_measure_blocks(H);
    if (H->dim == 2) {
        if (H->have_field) hipLaunchKernelGGL((k12_measure<2, true>), dim3(blocks), dim3(256), 0, ctx->stream, m);
        else hipLaunchKernelGGL((k12_measure<2, false>), dim3(blocks), dim3(256), 0, ctx->stream, m);
    } else {
        if (H->have_field) hipLaunchKernelGGL((k12_measure<3, true>), dim3(blocks), dim3(256), 0, ctx->stream, m);
        else hipLaunchKernelGGL((k12_measure<3, false>), dim3(blocks), dim3(256), 0, ctx->stream, m);
    }
    hipLaunchKernelGGL(energy_final, dim3(1), dim3(256), 0, ctx->stream, H->d_part, (int)blocks,
                       reinterpret_cast<double*>(d_row + TSU_POTTS_RECORD_WORDS));
    TSU_HIP_TRY(ctx, hipGetLastError());
    H->launches += 2;
    return TSU_OK;
}

template <int DIM>
int pd_run(tsu_potts_dis* H, double T, int n_meas, int sweeps_between, bool hb, uint64_t seed, uint32_t counter0, uint32_t replica) {
    using Sw = PdSw<DIM>;
    for (int k = 0; k < n_meas; ++k) {
        const uint32_t c0 = counter0 + (uint32_t)((long long)k * sweeps_between);
        int rc = hb ? pd_hb_sweep<DIM>(H, T, sweeps_between, seed, c0, replica) : sw_sweep<Sw>(H, {T}, sweeps_between, seed, c0, replica);
        if (rc == TSU_OK) rc = pd_measure_into(H, H->d_rec + (size_t)k * TSU_POTTS_DIS_RECORD_WORDS);
        if (rc != TSU_OK) return rc;
        H->rec_rows = k + 1;
    }
    return TSU_OK;
}

}  // namespace

extern "C" {

int tsu_potts_dis_site_thresholds(int q, const double* a, double T, uint64_t* thr) {
    if (!a || !thr || q < 2 || q > TSU_POTTS_MAX_Q || !isfinite(T) || !(T > 0.0)) return TSU_E_INVALID;
    double av[TSU_POTTS_MAX_Q] = {};
    for (int c = 0; c < q; ++c) {
        if (!isfinite(a[c])) return TSU_E_INVALID;
        av[c] = a[c];
    }
    uint64_t t[TSU_POTTS_MAX_Q];
    pd_thresholds(q, av, T, t);
    for (int c = 0; c < q; ++c) thr[c] = t[c];
    return TSU_OK;
}

int tsu_potts_dis_create(tsu_ctx* ctx, int depth, int rows, int cols, int q, const int* periodic, tsu_potts_dis** out) {
    TSU_ENTER(ctx);
    if (!ctx || !out) return TSU_E_INVALID;
    TSU_REQUIRE(ctx, periodic, "potts_dis_create: periodic is NULL");
    const int pz = periodic[0] != 0, pr = periodic[1] != 0, pc = periodic[2] != 0;
    TSU_REQUIRE(ctx, q >= 2 && q <= TSU_POTTS_MAX_Q, "potts_dis_create: q must be in 2 .. 8 (got %d)", q);
    TSU_REQUIRE(ctx, depth >= 1 && rows >= 1 && cols >= 1, "potts_dis_create: depth, rows and cols must be >= 1");
    TSU_REQUIRE(ctx, (long long)depth * rows < (1ll << 31) && (long long)depth * rows * cols < (1ll << 31),
                "potts_dis_create: %lld x %d sites exceed 32-bit labels", (long long)depth * rows, cols);
    TSU_REQUIRE(ctx, (!pz || (depth & 1) == 0) && (!pr || (rows & 1) == 0) && (!pc || (cols & 1) == 0),
                "potts_dis_create: a periodic axis needs an even length");
    tsu_potts_dis* H = new tsu_potts_dis();
    H->ctx = ctx;
    H->g = PottsGeom{depth, pz, pc, rows, cols, pr};
    H->dim = depth == 1 && !pz ? 2 : 3;
    H->q = q;
    H->m.q = q;
    H->m.sites = pd_sites(H);
    const size_t n = (size_t)pd_sites(H);
    hipError_t e = hipMalloc((void**)&H->d_s, n);
    if (e == hipSuccess) e = hipMalloc((void**)&H->d_obs, TSU_POTTS_DIS_RECORD_WORDS * sizeof(long long));
    if (e == hipSuccess) e = hipMalloc((void**)&H->d_part, kEnergyBlocks * sizeof(double));
    if (e == hipSuccess) e = hipMemsetAsync(H->d_s, 0, n, ctx->stream);
    if (e != hipSuccess) {
        if (H->d_s) (void)hipFree(H->d_s);
        if (H->d_obs) (void)hipFree(H->d_obs);
        if (H->d_part) (void)hipFree(H->d_part);
        delete H;
        return tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "potts_dis_create: %s", hipGetErrorString(e));
    }
    *out = H;
    return TSU_OK;
}

int tsu_potts_dis_destroy(tsu_potts_dis* H) {
    TSU_ENTER(H ? H->ctx : nullptr);
    if (!H) return TSU_E_INVALID;
    (void)hipStreamSynchronize(H->ctx->stream);
    (void)hipFree(H->d_s);
    (void)hipFree(H->d_obs);
    (void)hipFree(H->d_part);
    if (H->d_dis) (void)hipFree(H->d_dis);
    if (H->d_rec) (void)hipFree(H->d_rec);
    if (H->h_err) (void)hipHostFree(H->h_err);
    tsu_sw_scratch_free(H->sw);
    delete H;
    return TSU_OK;
}

int tsu_potts_dis_set_disorder(tsu_potts_dis* H, const float* J_right, const float* J_down, const float* J_layer, const float* h) {
    TSU_ENTER(H ? H->ctx : nullptr);
    if (!H) return TSU_E_INVALID;
    tsu_ctx* ctx = H->ctx;
    TSU_REQUIRE(ctx, J_right && J_down, "potts_dis_set_disorder: J_right and J_down are required");
    // a 2-D lattice given with a J_layer holds the open z axis's last (only) layer, which must be 0 as on any open axis; it is not stored
    TSU_REQUIRE(ctx, H->dim == 2 || J_layer, "potts_dis_set_disorder: a 3-D lattice needs J_layer");
    const int depth = H->g.depth, rows = H->g.rows, cols = H->g.cols;
    const size_t n = (size_t)pd_sites(H);
    bool nonneg = true;
    for (int z = 0; z < depth; ++z)
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) {
                const size_t i = ((size_t)z * rows + r) * cols + c;
                const float jl = J_layer ? J_layer[i] : 0.0f;
                TSU_REQUIRE(ctx, isfinite(J_right[i]) && isfinite(J_down[i]) && isfinite(jl),
                            "potts_dis_set_disorder: non-finite coupling at site (%d, %d, %d)", z, r, c);
                TSU_REQUIRE(ctx, H->g.pc || c + 1 < cols || J_right[i] == 0.0f,
                            "potts_dis_set_disorder: open axis: J_right[%d, %d, %d] (last column) must be 0, got %g", z, r, c, (double)J_right[i]);
                TSU_REQUIRE(ctx, H->g.pr || r + 1 < rows || J_down[i] == 0.0f,
                            "potts_dis_set_disorder: open axis: J_down[%d, %d, %d] (last row) must be 0, got %g", z, r, c, (double)J_down[i]);
                TSU_REQUIRE(ctx, H->g.pz || z + 1 < depth || jl == 0.0f,
                            "potts_dis_set_disorder: open axis: J_layer[%d, %d, %d] (last layer) must be 0, got %g", z, r, c, (double)jl);
                nonneg = nonneg && J_right[i] >= 0.0f && J_down[i] >= 0.0f && jl >= 0.0f;
            }
    bool zero_field = true;
    if (h)
        for (size_t i = 0; i < n * (size_t)H->q; ++i) {
            TSU_REQUIRE(ctx, isfinite(h[i]), "potts_dis_set_disorder: non-finite field at colour %zu, site %zu", i / n, i % n);
            zero_field = zero_field && h[i] == 0.0f;
        }
    const int nj = H->dim == 2 ? 2 : 3;
    if (!H->d_dis) TSU_HIP_TRY(ctx, hipMalloc((void**)&H->d_dis, (size_t)(nj + H->q) * n * sizeof(float)));
    const float* src[3] = {J_right, J_down, J_layer};
    for (int k = 0; k < nj; ++k)
        TSU_HIP_TRY(ctx, hipMemcpyAsync(H->d_dis + (size_t)k * n, src[k], n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    if (h) TSU_HIP_TRY(ctx, hipMemcpyAsync(H->d_dis + (size_t)nj * n, h, (size_t)H->q * n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    H->m.jr = H->d_dis;
    H->m.jd = H->d_dis + n;
    H->m.jl = H->dim == 2 ? nullptr : H->d_dis + 2 * n;
    H->m.h = h ? H->d_dis + (size_t)nj * n : nullptr;
    H->have_disorder = 1;
    H->have_field = h != nullptr;
    H->sw_ok = nonneg && zero_field;
    return TSU_OK;
}

int tsu_potts_dis_set_spins(tsu_potts_dis* H, const int8_t* colours) {
    TSU_ENTER(H ? H->ctx : nullptr);
    if (!H) return TSU_E_INVALID;
    tsu_ctx* ctx = H->ctx;
    TSU_REQUIRE(ctx, colours, "potts_dis_set_spins: colours is NULL");
    const size_t n = (size_t)pd_sites(H);
    for (size_t i = 0; i < n; ++i)
        TSU_REQUIRE(ctx, colours[i] >= 0 && colours[i] < H->q, "potts_dis_set_spins: colour %d at site %zu is outside 0 .. %d", (int)colours[i], i,
                    H->q - 1);
    TSU_HIP_TRY(ctx, hipMemcpyAsync(H->d_s, colours, n, hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int tsu_potts_dis_get_spins(tsu_potts_dis* H, int8_t* colours) {
    TSU_ENTER(H ? H->ctx : nullptr);
    if (!H) return TSU_E_INVALID;
    tsu_ctx* ctx = H->ctx;
    TSU_REQUIRE(ctx, colours, "potts_dis_get_spins: colours is NULL");
    TSU_HIP_TRY(ctx, hipMemcpyAsync(colours, H->d_s, (size_t)pd_sites(H), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return pd_check_err(H);
}

int tsu_potts_dis_fill(tsu_potts_dis* H, int colour) {
    TSU_ENTER(H ? H->ctx : nullptr);
    if (!H) return TSU_E_INVALID;
    TSU_REQUIRE(H->ctx, colour >= 0 && colour < H->q, "potts_dis_fill: colour %d is outside 0 .. %d", colour, H->q - 1);
    TSU_HIP_TRY(H->ctx, hipMemsetAsync(H->d_s, colour, (size_t)pd_sites(H), H->ctx->stream));
    return TSU_OK;
}

int tsu_potts_dis_sweep(tsu_potts_dis* H, double T, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica) {
    TSU_ENTER(H ? H->ctx : nullptr);
    if (!H) return TSU_E_INVALID;
    const int rc = pd_hb_check(H, T, n_sweeps, replica);
    if (rc != TSU_OK) return rc;
    return H->dim == 2 ? pd_hb_sweep<2>(H, T, n_sweeps, seed, sweep0, replica) : pd_hb_sweep<3>(H, T, n_sweeps, seed, sweep0, replica);
}

int tsu_potts_dis_cluster_sweep(tsu_potts_dis* H, double T, int n_steps, uint64_t seed, uint32_t step0, uint32_t replica) {
    TSU_ENTER(H ? H->ctx : nullptr);
    if (!H) return TSU_E_INVALID;
    return H->dim == 2 ? sw_sweep<PdSw<2>>(H, {T}, n_steps, seed, step0, replica) : sw_sweep<PdSw<3>>(H, {T}, n_steps, seed, step0, replica);
}

int tsu_potts_dis_route(tsu_potts_dis* H, int algorithm, int* route) {
    TSU_ENTER(H ? H->ctx : nullptr);
    if (!H || !route) return TSU_E_INVALID;
    TSU_REQUIRE(H->ctx, algorithm == TSU_POTTS_HEAT_BATH || algorithm == TSU_POTTS_SWENDSEN_WANG, "potts_dis_route: unknown algorithm %d", algorithm);
    if (algorithm == TSU_POTTS_HEAT_BATH) {
        *route = pd_hb_small_route(H) ? TSU_POTTS_DIS_ROUTE_SMALL : TSU_POTTS_DIS_ROUTE_SWEEP;
    } else {
        const bool small = H->dim == 2 ? sw_small_route<PdSw<2>>(H) : sw_small_route<PdSw<3>>(H);
        *route = small ? TSU_POTTS_DIS_ROUTE_SW_SMALL : TSU_POTTS_DIS_ROUTE_SW_TILES;
    }
    return TSU_OK;
}

int tsu_potts_dis_measure(tsu_potts_dis* H, int64_t* row, double* E) {
    TSU_ENTER(H ? H->ctx : nullptr);
    if (!H) return TSU_E_INVALID;
    tsu_ctx* ctx = H->ctx;
    TSU_REQUIRE(ctx, row, "potts_dis_measure: row is NULL");
    TSU_REQUIRE(ctx, !E || H->have_disorder, "potts_dis_measure: the energy needs tsu_potts_dis_set_disorder first");
    const int rc = pd_measure_into(H, H->d_obs);
    if (rc != TSU_OK) return rc;
    int64_t host[TSU_POTTS_DIS_RECORD_WORDS];
    TSU_HIP_TRY(ctx, hipMemcpyAsync(host, H->d_obs, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(row, host, TSU_POTTS_RECORD_WORDS * sizeof(int64_t));
    if (E) memcpy(E, host + TSU_POTTS_RECORD_WORDS, sizeof(double));
    return pd_check_err(H);
}

int tsu_potts_dis_run(tsu_potts_dis* H, double T, int n_meas, int sweeps_between, int algorithm, uint64_t seed, uint32_t counter0,
                      uint32_t replica) {
    TSU_ENTER(H ? H->ctx : nullptr);
    if (!H) return TSU_E_INVALID;
    tsu_ctx* ctx = H->ctx;
    const bool hb = algorithm == TSU_POTTS_HEAT_BATH;
    TSU_REQUIRE(ctx, hb || algorithm == TSU_POTTS_SWENDSEN_WANG, "potts_dis_run: unknown algorithm %d", algorithm);
    TSU_REQUIRE(ctx, n_meas >= 0 && sweeps_between >= 0, "potts_dis_run: n_meas and sweeps_between must be >= 0");
    const long long total = (long long)n_meas * sweeps_between;
    TSU_REQUIRE(ctx, total <= (1ll << 31), "potts_dis_run: %lld updates exceed one call", total);
    int rc;
    if (hb) rc = pd_hb_check(H, T, sweeps_between, replica);
    else rc = H->dim == 2 ? sw_check_call<PdSw<2>>(H, {T}, 0, counter0, replica) : sw_check_call<PdSw<3>>(H, {T}, 0, counter0, replica);
    if (rc != TSU_OK) return rc;
    TSU_REQUIRE(ctx, hb || (uint64_t)counter0 + (uint64_t)total <= (1ull << 32), "potts_dis_run: step counter overflow");
    const size_t bytes = (size_t)n_meas * TSU_POTTS_DIS_RECORD_WORDS * sizeof(long long);
    TSU_HIP_TRY(ctx, ising2d_grow(H->d_rec, H->rec_cap, bytes ? bytes : sizeof(long long)));
    H->rec_rows = 0;
    return H->dim == 2 ? pd_run<2>(H, T, n_meas, sweeps_between, hb, seed, counter0, replica)
                       : pd_run<3>(H, T, n_meas, sweeps_between, hb, seed, counter0, replica);
}

int tsu_potts_dis_record(tsu_potts_dis* H, int64_t* rows, int max_rows, int* n_rows) {
    TSU_ENTER(H ? H->ctx : nullptr);
    if (!H) return TSU_E_INVALID;
    tsu_ctx* ctx = H->ctx;
    TSU_REQUIRE(ctx, n_rows && max_rows >= 0 && (rows || max_rows == 0), "potts_dis_record: n_rows is NULL, max_rows negative or rows NULL");
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const int rc = pd_check_err(H);
    if (rc != TSU_OK) return rc;
    *n_rows = H->rec_rows;
    const int n = H->rec_rows < max_rows ? H->rec_rows : max_rows;
    if (n > 0) TSU_HIP_TRY(ctx, hipMemcpy(rows, H->d_rec, (size_t)n * TSU_POTTS_DIS_RECORD_WORDS * sizeof(int64_t), hipMemcpyDeviceToHost));
    return TSU_OK;
}

int tsu_potts_dis_launch_count(tsu_potts_dis* H, uint64_t* n) {
    TSU_ENTER(H ? H->ctx : nullptr);
    if (!H || !n) return TSU_E_INVALID;
    *n = H->launches + H->sw.launches;
    return TSU_OK;
}

}  // extern "C"

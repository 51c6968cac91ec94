// pop_host.h -- the host side of a population-annealing handle, once for the 2-D populations (tsu_pa2d, ising2d_disorder.hip) and the
// 3-D populations (tsu_pa3d, ising3d.hip): free functions on pop_handle, which holds what both have.  A handle type derives from it
// (plain struct inheritance) and adds `lat`, the one lattice handle that owns the disorder.  The dimension passes in how it launches
// a half-sweep and an energy partial pass (the ladders' kernels, unchanged: every walker sits at slot 0 and the kernels get the
// schedule's tables offset by the step); create, set_schedule, init, the run loop, history, energies and spins are here.  Messages
// carry the handle's name ("pa2d" / "pa3d") as their prefix.  Internal linkage throughout, as pop_dev.h.
//
// Memory: all R spin planes are one allocation (R nrows pitch bytes) with a device table of the planes' addresses beside it; the
// energy partials keep the kernels' fixed stride of kEnergyBlocks per walker (16 KiB per walker for E and sum of spins together,
// 1 GiB at R = 65535).
//
// Overlaps of walker pairs (set_overlap; DESIGN.md section 3, "Overlaps of walker pairs"): the pairs are (i, i + P), P = R / 2, and the
// ladders' passes compute them as they stand: pt_overlap, pt_link, pt_profile and pt_modes find their two planes as
// s[was[i]] and s[R' + was[R' + i]], so with R' := P and the table was = (0 .. P - 1, 0 .. P - 1) they read walkers i and P + i.
#pragma once
#include <cmath>
#include <new>
#include <vector>

#include "pop_dev.h"
#include "pt_host.h"

constexpr int kPopMaxSteps = 1 << 20;

struct pop_handle {
    tsu_ctx* ctx;
    const char* name;              // "pa2d" / "pa3d": the prefix of the messages
    int R, K;                      // walkers; steps of the schedule (K + 1 inverse temperatures)
    int have_sched, have_init, have_E;  // have_E: d_E / d_M belong to the planes as they are
    uint32_t sweeps, step;         // sweeps of every walker and steps since init
    unsigned long long launches;   // half-sweep launches
    int hist_steps, hist_resampled;  // steps recorded by the last run, and whether it resampled (W, S, U, E_min recorded)
    size_t hist_cap;               // steps the history buffers hold
    long long nrows, pitch;        // a walker's spin plane: nrows rows of pitch bytes, the first cols of each counting
    int cols;
    size_t plane;                  // nrows * pitch
    int8_t* d_pool;                // the R planes
    int8_t** d_s;                  // walker -> its plane
    uint32_t* d_key;               // walker -> (k0, k1) of seed + walker
    int32_t* d_slot;               // walker -> 0
    double* d_T;                   // step -> 1 / beta
    float* d_c32;                  // step -> fl32(2 / T)
    double* d_part;                // [walker][kEnergyBlocks] energy partials
    long long* d_ipart;            // [walker][kEnergyBlocks] sum-of-spin partials
    double* d_E;                   // walker -> E of the last energy pass
    long long* d_M;                // walker -> sum of spins
    uint32_t* d_W;                 // plan scratch: the rows of a run that does not record
    int32_t* d_parent;
    uint32_t* d_xs;                // [R + 1]
    int32_t* d_dead;               // [R]
    int2* d_pairs;                 // [R]
    uint32_t* d_npairs;
    double* d_hE;                  // [step + 1][walker]
    long long* d_hM;
    uint32_t* d_hW;                // [step][walker]
    int32_t* d_hP;
    unsigned long long* d_hS;      // [step]
    unsigned long long* d_hU;
    double* d_hEmin;
    uint32_t key0, key1;           // Philox key of the resampling offset (the seed)
    // overlaps of the walker pairs: the lattice's axes as the handle's create fills them in, then what set_overlap adds
    int n_axes, lrows;             // axes (2 or 3) and the rows of a layer (2-D: nrows)
    int axis_len[3], axis_per[3];  // length and periodic flag per axis, in axis order
    int ovl, ovl_modes;            // a recording run also records q and L per pair / and the k_min modes
    int hist_ovl, hist_ovl_modes;  // the last run's rows have them
    int32_t* d_was;                // [2][P] -> 0 .. P - 1: the slot table that makes the ladders' passes read the pairs
    long long* d_prof;             // [pair][sum of axis_len] profile scratch
    double* d_tab;                 // per periodic axis, in axis order: cos[len], sin[len]
    long long* d_hq;               // [step + 1][pair]
    long long* d_hL;
    double* d_hF;                  // [step + 1][pair][periodic axis][re, im]
    std::vector<double> beta;      // host copy of the schedule
};

namespace {

void pop_free_history(pop_handle* P) {
    void* bufs[] = {P->d_hE, P->d_hM, P->d_hW, P->d_hP, P->d_hS, P->d_hU, P->d_hEmin, P->d_hq, P->d_hL, P->d_hF};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    P->d_hE = nullptr;
    P->d_hM = nullptr;
    P->d_hW = nullptr;
    P->d_hP = nullptr;
    P->d_hS = nullptr;
    P->d_hU = nullptr;
    P->d_hEmin = nullptr;
    P->d_hq = nullptr;
    P->d_hL = nullptr;
    P->d_hF = nullptr;
    P->hist_cap = 0;
}

// the handle with its planes, tables and history, and its lattice (destroy(lat) frees it)
template <class H, class Destroy>
void pop_delete(H* P, Destroy destroy) {
    void* bufs[] = {P->d_pool, P->d_s, P->d_key, P->d_slot, P->d_T, P->d_c32, P->d_part, P->d_ipart, P->d_E,
                    P->d_M, P->d_W, P->d_parent, P->d_xs, P->d_dead, P->d_pairs, P->d_npairs, P->d_was, P->d_prof, P->d_tab};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    pop_free_history(P);
    if (P->lat) (void)destroy(P->lat);
    delete P;
}

// the planes and tables of a population whose shape is known (synchronises)
int pop_alloc(pop_handle* P) {
    tsu_ctx* ctx = P->ctx;
    const size_t R = (size_t)P->R;
    P->plane = (size_t)P->nrows * (size_t)P->pitch;
    TSU_REQUIRE(ctx, P->pitch % 16 == 0 && P->plane / 16 < (1ull << 32), "%s_create: a plane of %zu bytes is too large", P->name, P->plane);
    hipError_t e = hipSuccess;
    auto alloc = [&e](auto*& ptr, size_t bytes) {
        if (e == hipSuccess) e = hipMalloc((void**)&ptr, bytes);
    };
    alloc(P->d_pool, R * P->plane);
    alloc(P->d_s, R * sizeof(int8_t*));
    alloc(P->d_key, 2 * R * sizeof(uint32_t));
    alloc(P->d_slot, R * sizeof(int32_t));
    alloc(P->d_part, R * kEnergyBlocks * sizeof(double));
    alloc(P->d_ipart, R * kEnergyBlocks * sizeof(long long));
    alloc(P->d_E, R * sizeof(double));
    alloc(P->d_M, R * sizeof(long long));
    alloc(P->d_W, R * sizeof(uint32_t));
    alloc(P->d_parent, R * sizeof(int32_t));
    alloc(P->d_xs, (R + 1) * sizeof(uint32_t));
    alloc(P->d_dead, R * sizeof(int32_t));
    alloc(P->d_pairs, R * sizeof(int2));
    alloc(P->d_npairs, sizeof(uint32_t));
    std::vector<int8_t*> planes(R);
    for (size_t g = 0; g < R; ++g) planes[g] = P->d_pool + g * P->plane;
    if (e == hipSuccess) e = hipMemsetAsync(P->d_pool, 0, R * P->plane, ctx->stream);  // pad bytes stay 0
    if (e == hipSuccess) e = hipMemcpyAsync(P->d_s, planes.data(), R * sizeof(int8_t*), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(P->d_key, 0, 2 * R * sizeof(uint32_t), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(P->d_slot, 0, R * sizeof(int32_t), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(P->d_npairs, 0, sizeof(uint32_t), ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // before `planes` goes
    if (e != hipSuccess) {
        const int rc = tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "%s_create: population of %d planes of %zu bytes: %s",
                                P->name, P->R, P->plane, hipGetErrorString(e));
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    return TSU_OK;
}

// create: the checks, the handle H (a pop_handle with the lattice `lat`), make(P) creates the lattice (its own shape checks and
// messages) and fills nrows / pitch / cols, then the planes and tables.  A population that does not fit leaves nothing behind
// (free_handle(P)), HIP's last error included.
template <class H, class Make, class Free>
int pop_create(tsu_ctx* ctx, const char* name, int population, H** out, Make make, Free free_handle) {
    *out = nullptr;
    TSU_REQUIRE(ctx, population >= 2 && population <= kPopMaxWalkers, "%s_create: population must be in [2, %d], got %d", name, kPopMaxWalkers,
                population);
    H* P = new (std::nothrow) H();
    if (!P) return tsu_fail(ctx, TSU_E_NOMEM, "%s_create: host allocation failed", name);
    P->ctx = ctx;
    P->name = name;
    P->R = population;
    int rc = make(P);
    if (rc == TSU_OK) rc = pop_alloc(P);
    if (rc != TSU_OK) {
        free_handle(P);
        (void)hipGetLastError();
        return rc;
    }
    *out = P;
    return TSU_OK;
}

// lanes of a pass over one walker: a lane per chunk of 16 columns
long long pop_lanes(const pop_handle* P) { return P->nrows * ((P->cols + 15) / 16); }

// walkers per lane of the sweeps: the ladders' rule
int pop_group(const pop_handle* P) { return pt_group_of(P->ctx, pop_lanes(P), P->R); }

// the schedule beta[0] < .. < beta[n - 1], beta[0] >= 0; the population has to be initialised again afterwards (synchronises)
int pop_set_schedule(pop_handle* P, const double* betas, int n) {
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, betas, "%s_set_schedule: NULL betas", P->name);
    TSU_REQUIRE(ctx, n >= 2 && n - 1 <= kPopMaxSteps, "%s_set_schedule: need 2 to %d inverse temperatures, got %d", P->name, kPopMaxSteps + 1, n);
    TSU_REQUIRE(ctx, betas[0] >= 0.0 && std::isfinite(betas[0]), "%s_set_schedule: beta[0] must be finite and >= 0, got %g", P->name, betas[0]);
    for (int k = 1; k < n; ++k)
        TSU_REQUIRE(ctx, std::isfinite(betas[k]) && betas[k] > betas[k - 1], "%s_set_schedule: betas must increase (beta[%d] = %g after %g)",
                    P->name, k, betas[k], betas[k - 1]);
    std::vector<double> t((size_t)n);
    std::vector<float> c((size_t)n);
    for (int k = 0; k < n; ++k) {
        t[k] = 1.0 / betas[k];  // +inf at beta = 0: no sweep runs there
        c[k] = (float)(2.0 / t[k]);
    }
    double* dT = nullptr;
    float* dc = nullptr;
    hipError_t e = hipMalloc((void**)&dT, (size_t)n * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&dc, (size_t)n * sizeof(float));
    if (e == hipSuccess) e = hipMemcpyAsync(dT, t.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dc, c.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // also: no kernel still reads the old tables
    if (e != hipSuccess) {
        if (dT) (void)hipFree(dT);
        if (dc) (void)hipFree(dc);
        (void)hipGetLastError();
        return tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "%s_set_schedule: %s", P->name, hipGetErrorString(e));
    }
    if (P->d_T) (void)hipFree(P->d_T);
    if (P->d_c32) (void)hipFree(P->d_c32);
    P->d_T = dT;
    P->d_c32 = dc;
    P->beta.assign(betas, betas + n);
    P->K = n - 1;
    P->have_sched = 1;
    P->have_init = 0;
    P->step = 0;
    return TSU_OK;
}

// every walker's E and sum of spins into E / M (asynchronous); partials(blocks) enqueues the dimension's partial pass
template <class Partials>
void pop_enqueue_energies(pop_handle* P, Partials&& partials, double* E, long long* M) {
    const unsigned blocks = reduce_blocks(pop_lanes(P));
    partials(blocks);
    pt_energy_final<<<(unsigned)P->R, 256, 0, P->ctx->stream>>>(P->d_part, P->d_ipart, (int)blocks, E, M);
}

// theta sweeps of every walker at step k's temperature: sweep(hs, colour, k) enqueues half-sweep hs
template <class Sweep>
void pop_sweeps(pop_handle* P, int theta, int k, Sweep&& sweep) {
    for (int s = 0; s < theta; ++s)
        for (int colour = 0; colour < 2; ++colour) {
            sweep(2u * (P->sweeps + (uint32_t)s) + (uint32_t)colour, colour, k);
            P->launches += 1;
        }
    P->sweeps += (uint32_t)theta;
}

// init: walker i gets the key seed + i and the single lattice's random start of that seed, the counters return to 0, then, if
// beta[0] > 0, initial_sweeps sweeps at 1 / beta[0], and the energies.  Nothing here waits for the device but the key upload.
template <class Sweep, class Partials>
int pop_init(pop_handle* P, int have_disorder, uint64_t seed, int initial_sweeps, Sweep&& sweep, Partials&& partials) {
    tsu_ctx* ctx = P->ctx;
    const char* nm = P->name;
    TSU_REQUIRE(ctx, have_disorder, "%s_init: call tsu_%s_set_disorder first", nm, nm);
    TSU_REQUIRE(ctx, P->have_sched, "%s_init: call tsu_%s_set_schedule first", nm, nm);
    TSU_REQUIRE(ctx, initial_sweeps >= 0, "%s_init: initial_sweeps must be >= 0, got %d", nm, initial_sweeps);
    P->have_init = 0;
    std::vector<uint32_t> key(2 * (size_t)P->R);
    for (int g = 0; g < P->R; ++g) {
        const uint64_t s = seed + (uint64_t)g;
        key[2 * g] = (uint32_t)s;
        key[2 * g + 1] = (uint32_t)(s >> 32);
    }
    TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_key, key.data(), key.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    const long long lanes = pop_lanes(P);
    pop_randomize<<<dim3((unsigned)((lanes + 255) / 256), (unsigned)P->R, 1), 256, 0, ctx->stream>>>(P->d_s, seed, P->nrows, P->pitch, P->cols);
    TSU_HIP_TRY(ctx, hipGetLastError());
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // before `key` goes
    P->sweeps = 0;
    P->step = 0;
    P->hist_steps = 0;
    P->key0 = (uint32_t)seed;
    P->key1 = (uint32_t)(seed >> 32);
    if (P->beta[0] > 0.0) pop_sweeps(P, initial_sweeps, 0, sweep);
    pop_enqueue_energies(P, partials, P->d_E, P->d_M);
    TSU_HIP_TRY(ctx, hipGetLastError());
    P->have_E = 1;
    P->have_init = 1;
    return TSU_OK;
}

// what a run needs, in the order the messages are promised
int pop_run_check(pop_handle* P, int have_disorder, int n_steps, int sweeps_per_step) {
    tsu_ctx* ctx = P->ctx;
    const char* nm = P->name;
    TSU_REQUIRE(ctx, have_disorder, "%s_run: call tsu_%s_set_disorder first", nm, nm);
    TSU_REQUIRE(ctx, P->have_sched, "%s_run: call tsu_%s_set_schedule first", nm, nm);
    TSU_REQUIRE(ctx, P->have_init, "%s_run: call tsu_%s_init first", nm, nm);
    TSU_REQUIRE(ctx, n_steps >= 0 && sweeps_per_step >= 0, "%s_run: need n_steps >= 0 and sweeps_per_step >= 0 (got %d, %d)", nm, n_steps,
                sweeps_per_step);
    TSU_REQUIRE(ctx, (uint64_t)P->step + (uint64_t)n_steps <= (uint64_t)P->K,
                "%s_run: %d steps from step %u run past the schedule of %d steps", nm, n_steps, P->step, P->K);
    TSU_REQUIRE(ctx, (uint64_t)P->sweeps + (uint64_t)n_steps * (uint64_t)sweeps_per_step <= (1ull << 31), "%s_run: sweep counter overflow", nm);
    return TSU_OK;
}

// n_steps steps after pop_run_check.  A step: the plan and the copy (if it resamples), sweeps_per_step sweeps at the step's
// temperature, one energy pass (the row of the record, and the next step's weights).  Nothing here waits for the device.
template <class Sweep, class Partials>
int pop_run(pop_handle* P, int n_steps, int theta, int resample, int record, Sweep&& sweep, Partials&& partials) {
    tsu_ctx* ctx = P->ctx;
    const size_t R = (size_t)P->R, n = (size_t)n_steps, np = R / 2;
    if (record && (P->hist_cap < n || !P->d_hE)) {
        pop_free_history(P);
        const size_t cap = n ? n : 1;
        hipError_t e = hipMalloc((void**)&P->d_hE, (cap + 1) * R * sizeof(double));
        if (e == hipSuccess) e = hipMalloc((void**)&P->d_hM, (cap + 1) * R * sizeof(long long));
        if (e == hipSuccess) e = hipMalloc((void**)&P->d_hW, cap * R * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc((void**)&P->d_hP, cap * R * sizeof(int32_t));
        if (e == hipSuccess) e = hipMalloc((void**)&P->d_hS, cap * sizeof(unsigned long long));
        if (e == hipSuccess) e = hipMalloc((void**)&P->d_hU, cap * sizeof(unsigned long long));
        if (e == hipSuccess) e = hipMalloc((void**)&P->d_hEmin, cap * sizeof(double));
        if (e == hipSuccess && P->ovl) e = hipMalloc((void**)&P->d_hq, (cap + 1) * np * sizeof(long long));
        if (e == hipSuccess && P->ovl) e = hipMalloc((void**)&P->d_hL, (cap + 1) * np * sizeof(long long));
        if (e == hipSuccess && P->ovl_modes) e = hipMalloc((void**)&P->d_hF, (cap + 1) * np * pt_mode_doubles(P) * sizeof(double));
        if (e != hipSuccess) {  // nothing of a history that does not fit stays behind
            pop_free_history(P);
            P->hist_steps = 0;
            (void)hipGetLastError();
            return tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "%s_run: history of %d steps: %s", P->name, n_steps,
                            hipGetErrorString(e));
        }
        P->hist_cap = cap;
    }
    P->hist_steps = record ? n_steps : -1;
    P->hist_resampled = record && resample;
    P->hist_ovl = record && P->ovl;
    P->hist_ovl_modes = record && P->ovl_modes;
    // the overlap rows of this run: pt_overlap and pt_link add into theirs, so q and L start at 0
    LinkArgs la;
    ProfArgs pa;
    ModeArgs ma = {};
    const unsigned lblocks = pt_link_plan(P, la), oblocks = reduce_blocks(pop_lanes(P));
    const dim3 pgrid = profile_plan(pa, P->pitch, P->pitch, P->nrows, P->lrows, P->cols, P->n_axes == 3, (unsigned)np);
    const long long plen = pt_prof_len(P);
    const size_t md = pt_mode_doubles(P);
    if (P->hist_ovl) {
        TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_hq, 0, (n + 1) * np * sizeof(long long), ctx->stream));
        TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_hL, 0, (n + 1) * np * sizeof(long long), ctx->stream));
        if (P->hist_ovl_modes) ma = pt_mode_args(P);
    }
    // row `row` of the overlap record from the planes as they are (asynchronous)
    auto overlaps = [&](size_t row) -> int {
        pt_overlap<<<dim3(oblocks, (unsigned)np, 1), 256, 0, ctx->stream>>>(P->d_s, P->d_was, (int)np, P->pitch, P->nrows, P->cols,
                                                                           P->d_hq + row * np);
        pt_link<<<dim3(lblocks, (unsigned)np, 1), 256, 0, ctx->stream>>>(P->d_s, P->d_was, (int)np, la, P->d_hL + row * np);
        if (P->hist_ovl_modes) {
            TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_prof, 0, np * (size_t)plen * sizeof(long long), ctx->stream));
            pt_profile<<<pgrid, 256, 0, ctx->stream>>>(P->d_s, P->d_was, (int)np, 2, pa, P->d_prof, plen);
            pt_modes<<<dim3(2u * (unsigned)ma.n, (unsigned)np, 1), 256, 0, ctx->stream>>>(P->d_prof, plen, ma, P->d_hF + row * np * md);
        }
        return TSU_OK;
    };
    if (P->hist_ovl) {
        const int rc = overlaps(0);
        if (rc != TSU_OK) return rc;
    }
    if (!P->have_E) {  // the planes or the disorder changed since the last pass
        pop_enqueue_energies(P, partials, P->d_E, P->d_M);
        P->have_E = 1;
    }
    if (record) {
        TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_hE, P->d_E, R * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_hM, P->d_M, R * sizeof(long long), hipMemcpyDeviceToDevice, ctx->stream));
        if (!resample && n) {
            pop_identity<<<(unsigned)((n * R + 255) / 256 < 1024 ? (n * R + 255) / 256 : 1024), 256, 0, ctx->stream>>>(P->d_hP, P->R,
                                                                                                                      (long long)(n * R));
            TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_hW, 0, n * R * sizeof(uint32_t), ctx->stream));
            TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_hS, 0, n * sizeof(unsigned long long), ctx->stream));
            TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_hU, 0, n * sizeof(unsigned long long), ctx->stream));
            TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_hEmin, 0, n * sizeof(double), ctx->stream));
        }
    }
    PopPlan pl;
    pl.xs = P->d_xs;
    pl.dead = P->d_dead;
    pl.pairs = P->d_pairs;
    pl.n_pairs = P->d_npairs;
    pl.R = P->R;
    pl.k0 = P->key0;
    pl.k1 = P->key1;
    const uint32_t cpp = (uint32_t)(P->plane / 16);
    const unsigned long long max_items = (unsigned long long)R * ((cpp + 255u) / 256u);
    const unsigned long long want = (unsigned long long)(ctx->cus > 0 ? ctx->cus : 256) * 8;
    const unsigned copy_grid = (unsigned)(max_items < want ? max_items : want);
    const double* curE = P->d_E;  // the energies the next plan reads: the last pass's row
    for (size_t j = 0; j < n; ++j) {
        const int k = (int)P->step + 1;
        if (resample) {
            pl.E = curE;
            pl.W = record ? P->d_hW + j * R : P->d_W;
            pl.parent = record ? P->d_hP + j * R : P->d_parent;
            pl.S = record ? P->d_hS + j : nullptr;
            pl.U = record ? P->d_hU + j : nullptr;
            pl.Emin = record ? P->d_hEmin + j : nullptr;
            pl.db = P->beta[k] - P->beta[k - 1];
            pl.k_abs = P->step;
            pop_plan<<<1, kPopPlanThreads, 0, ctx->stream>>>(pl);
            pop_copy<<<copy_grid, 256, 0, ctx->stream>>>(P->d_s, P->d_pairs, P->d_npairs, cpp);
        }
        pop_sweeps(P, theta, k, sweep);
        double* E = record ? P->d_hE + (j + 1) * R : P->d_E;
        pop_enqueue_energies(P, partials, E, record ? P->d_hM + (j + 1) * R : P->d_M);
        curE = E;
        P->step += 1;
        if (P->hist_ovl) {
            const int rc = overlaps(j + 1);
            if (rc != TSU_OK) return rc;
        }
    }
    if (record && n) {  // between runs the current energies live in d_E / d_M
        TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_E, P->d_hE + n * R, R * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_M, P->d_hM + n * R, R * sizeof(long long), hipMemcpyDeviceToDevice, ctx->stream));
    }
    TSU_HIP_TRY(ctx, hipGetLastError());  // one check for all the launches above: a launch that fails leaves its error for this call
    return TSU_OK;
}

// the last recording run's rows: E, M [n + 1][R]; W, parent [n][R]; S, U, E_min [n] (any may be NULL; synchronises).  A run that
// did not resample has parent = identity and W, S, U, E_min = 0.
int pop_history(pop_handle* P, double* E, int64_t* M, uint32_t* W, int32_t* parent, uint64_t* S, uint64_t* U, double* Emin) {
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, P->hist_steps >= 0 && P->d_hE, "%s_history: the last run recorded nothing", P->name);
    const size_t n = (size_t)P->hist_steps, R = (size_t)P->R;
    if (E) TSU_HIP_TRY(ctx, hipMemcpyAsync(E, P->d_hE, (n + 1) * R * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (M) TSU_HIP_TRY(ctx, hipMemcpyAsync(M, P->d_hM, (n + 1) * R * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (n) {
        if (W) TSU_HIP_TRY(ctx, hipMemcpyAsync(W, P->d_hW, n * R * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        if (parent) TSU_HIP_TRY(ctx, hipMemcpyAsync(parent, P->d_hP, n * R * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        if (S) TSU_HIP_TRY(ctx, hipMemcpyAsync(S, P->d_hS, n * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        if (U) TSU_HIP_TRY(ctx, hipMemcpyAsync(U, P->d_hU, n * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        if (Emin) TSU_HIP_TRY(ctx, hipMemcpyAsync(Emin, P->d_hEmin, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

// set_overlap: cs[a] / sn[a] = the host's cos / sin tables of axis a (all NULL: q and L only; else both NULL exactly on an open
// axis).  Switching it on, or changing whether the modes are recorded, drops the recorded history (its buffers gain the overlap rows
// with the next run); a buffer that does not fit leaves the handle as it was (synchronises)
int pop_set_overlap(pop_handle* P, int enable, const double* const* cs, const double* const* sn) {
    tsu_ctx* ctx = P->ctx;
    if (!enable) {
        P->ovl = P->ovl_modes = 0;
        return TSU_OK;
    }
    int given = 0;
    for (int a = 0; a < P->n_axes; ++a) given += (cs[a] || sn[a]) ? 1 : 0;
    size_t ntab = 0;
    if (given) {
        TSU_REQUIRE(ctx, pt_periodic_axes(P) > 0, "%s_set_overlap: the lattice has no periodic axis (no k_min mode is defined)", P->name);
        for (int a = 0; a < P->n_axes; ++a) {
            if (P->axis_per[a]) {
                TSU_REQUIRE(ctx, cs[a] && sn[a], "%s_set_overlap: NULL table of periodic axis %d", P->name, a);
                ntab += 2 * (size_t)P->axis_len[a];
            } else {
                TSU_REQUIRE(ctx, !cs[a] && !sn[a], "%s_set_overlap: axis %d is open: its tables must be NULL", P->name, a);
            }
        }
    }
    const size_t np = (size_t)P->R / 2;
    int32_t* was = nullptr;
    long long* prof = nullptr;
    double* tab = nullptr;
    hipError_t e = hipSuccess;
    if (!P->d_was) e = hipMalloc((void**)&was, 2 * np * sizeof(int32_t));
    if (e == hipSuccess && given && !P->d_prof) e = hipMalloc((void**)&prof, np * (size_t)pt_prof_len(P) * sizeof(long long));
    if (e == hipSuccess && given && !P->d_tab) e = hipMalloc((void**)&tab, ntab * sizeof(double));
    if (e != hipSuccess) {  // nothing of this call stays behind
        void* bufs[] = {was, prof, tab};
        for (void* b : bufs)
            if (b) (void)hipFree(b);
        (void)hipGetLastError();
        return tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "%s_set_overlap: scratch of %zu pairs: %s", P->name, np,
                        hipGetErrorString(e));
    }
    if (was) P->d_was = was;
    if (prof) P->d_prof = prof;
    if (tab) P->d_tab = tab;
    std::vector<int32_t> ident(2 * np);
    for (size_t i = 0; i < 2 * np; ++i) ident[i] = (int32_t)(i % np);
    TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_was, ident.data(), ident.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    if (given) {
        double* t = P->d_tab;
        for (int a = 0; a < P->n_axes; ++a)
            if (P->axis_per[a]) {
                const size_t len = (size_t)P->axis_len[a];
                TSU_HIP_TRY(ctx, hipMemcpyAsync(t, cs[a], len * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
                TSU_HIP_TRY(ctx, hipMemcpyAsync(t + len, sn[a], len * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
                t += 2 * len;
            }
    }
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // before `ident` and the caller's tables go; no kernel still writes the rows
    if (!P->ovl || P->ovl_modes != (given ? 1 : 0)) {
        pop_free_history(P);
        P->hist_steps = -1;
        P->hist_ovl = P->hist_ovl_modes = 0;
    }
    P->ovl = 1;
    P->ovl_modes = given ? 1 : 0;
    return TSU_OK;
}

// the last recording run's overlap rows: q, L [n + 1][P]; modes [n + 1][P][periodic axis][re, im] (any may be NULL; synchronises)
int pop_history_overlap(pop_handle* P, int64_t* q, int64_t* L, double* modes) {
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, P->hist_steps >= 0 && P->hist_ovl && P->d_hq,
                "%s_history_overlap: the last run recorded no overlaps (call tsu_%s_set_overlap before a recording run)", P->name, P->name);
    TSU_REQUIRE(ctx, !modes || P->hist_ovl_modes, "%s_history_overlap: the last run recorded no modes (tsu_%s_set_overlap was given no tables)",
                P->name, P->name);
    const size_t n = ((size_t)P->hist_steps + 1) * ((size_t)P->R / 2);
    if (q) TSU_HIP_TRY(ctx, hipMemcpyAsync(q, P->d_hq, n * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (L) TSU_HIP_TRY(ctx, hipMemcpyAsync(L, P->d_hL, n * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (modes) TSU_HIP_TRY(ctx, hipMemcpyAsync(modes, P->d_hF, n * pt_mode_doubles(P) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

// every walker's E and sum of spins now (synchronises)
template <class Partials>
int pop_energies(pop_handle* P, int have_disorder, double* E, int64_t* sum_s, Partials&& partials) {
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, have_disorder, "%s_energies: call tsu_%s_set_disorder first", P->name, P->name);
    TSU_REQUIRE(ctx, P->have_init, "%s_energies: call tsu_%s_init first", P->name, P->name);
    pop_enqueue_energies(P, partials, P->d_E, P->d_M);
    TSU_HIP_TRY(ctx, hipGetLastError());
    P->have_E = 1;
    if (E) TSU_HIP_TRY(ctx, hipMemcpyAsync(E, P->d_E, (size_t)P->R * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (sum_s) TSU_HIP_TRY(ctx, hipMemcpyAsync(sum_s, P->d_M, (size_t)P->R * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

// walker i's spins, nrows x cols int8 row-major on the host (synchronises)
int pop_get_spins(pop_handle* P, int i, int8_t* host) {
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, host, "%s_get_spins: NULL output", P->name);
    TSU_REQUIRE(ctx, i >= 0 && i < P->R, "%s_get_spins: walker %d out of range (population %d)", P->name, i, P->R);
    TSU_REQUIRE(ctx, P->have_init, "%s_get_spins: call tsu_%s_init first", P->name, P->name);
    TSU_HIP_TRY(ctx, hipMemcpy2DAsync(host, (size_t)P->cols, P->d_pool + (size_t)i * P->plane, (size_t)P->pitch, (size_t)P->cols,
                                      (size_t)P->nrows, hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int pop_set_spins(pop_handle* P, int i, const int8_t* host) {
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, host, "%s_set_spins: NULL input", P->name);
    TSU_REQUIRE(ctx, i >= 0 && i < P->R, "%s_set_spins: walker %d out of range (population %d)", P->name, i, P->R);
    TSU_REQUIRE(ctx, P->have_init, "%s_set_spins: call tsu_%s_init first", P->name, P->name);
    TSU_HIP_TRY(ctx, hipMemcpy2DAsync(P->d_pool + (size_t)i * P->plane, (size_t)P->pitch, host, (size_t)P->cols, (size_t)P->cols,
                                      (size_t)P->nrows, hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    P->have_E = 0;
    return TSU_OK;
}

int pop_launch_count(const pop_handle* P, uint64_t* n) {
    if (!P || !n) return TSU_E_INVALID;
    *n = P->launches;
    return TSU_OK;
}

}  // namespace

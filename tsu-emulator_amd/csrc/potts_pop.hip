// potts_pop.hip -- K14: population annealing of K12's Potts lattice (gfx950), the host side and the C ABI of
// include/tsu_hip_potts_pop.h; the contract is DESIGN.md section 3, "Population annealing of Potts lattices (K14)".  The kernels are
// potts_pop_kern_dev.h's, which run K12's octet bodies and measuring order per walker; the resampling is pop_dev.h's pop_plan and
// pop_copy as they stand, fed with a table of the walkers' addresses; the packing rule is potts_pop_plan.h's.  One handle serves
// both dimensions, as K12's and K13's do: depth 1 with an open z axis launches the DIM = 2 instantiations.
#include <math.h>
#include <stdlib.h>

#include <new>
#include <vector>

#include "potts_pop_kern_dev.h"

constexpr int kPottsPopMaxSteps = 1 << 20;

struct tsu_potts_pop {
    tsu_ctx* ctx;
    PottsGeom g;  // 2-D: depth 1, pz 0
    int dim, q, R, K;
    long long sites, stride, lanes;
    int8_t* d_pool;  // R walkers of `stride` bytes: one allocation, pad bytes 0
    int8_t** d_s;    // walker -> its colours (pop_copy's table)
    float* d_dis;    // J_right, J_down, J_layer (3-D), then the q colour planes of h (when given): one copy for all walkers
    PdModel m;
    int have_disorder, have_field, have_sched, have_init, have_E;
    uint32_t sweeps, offset, step;  // sweeps and steps since init; what advance added to the counter (wraps)
    uint64_t seed;
    unsigned long long launches;
    unsigned blocks;  // pd_measure_blocks of the shape
    double* d_part;               // [walker][blocks]
    unsigned long long* d_ipart;  // [walker][blocks][9]
    double* d_E;                  // walker -> E of the last measuring pass
    long long *d_neq, *d_N;       // walker -> n_eq; [walker][8] colour counts
    uint32_t* d_W;                // plan scratch: the rows of a run that does not record
    int32_t* d_parent;
    uint32_t* d_xs;
    int32_t* d_dead;
    int2* d_pairs;
    uint32_t* d_npairs;
    double* d_hE;                 // [step + 1][walker]
    long long *d_hM, *d_hN;       // n_eq [step + 1][walker]; N [step + 1][walker][8]
    uint32_t* d_hW;               // [step][walker]
    int32_t* d_hP;
    unsigned long long *d_hS, *d_hU;  // [step]
    double* d_hEmin;
    size_t hist_cap;
    int hist_steps;               // steps recorded by the last run (-1: it recorded nothing)
    std::vector<double> beta;
};

namespace {

bool ppop_env_off(const char* name) {  // <name>=0 (tests, read per call)
    const char* e = getenv(name);
    return e && atoi(e) == 0;
}

PottsPopPlan ppop_plan(const tsu_potts_pop* P) {
    return potts_pop_plan(P->sites, P->lanes, P->dim, P->q, P->have_field, P->R, !ppop_env_off("TSU_POTTS_POP_PACK"),
                          !ppop_env_off("TSU_POTTS_SMALL"));
}

void ppop_free_history(tsu_potts_pop* P) {
    void* bufs[] = {P->d_hE, P->d_hM, P->d_hN, P->d_hW, P->d_hP, P->d_hS, P->d_hU, P->d_hEmin};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    P->d_hE = nullptr;
    P->d_hM = P->d_hN = nullptr;
    P->d_hW = nullptr;
    P->d_hP = nullptr;
    P->d_hS = P->d_hU = nullptr;
    P->d_hEmin = nullptr;
    P->hist_cap = 0;
    P->hist_steps = -1;
}

void ppop_free(tsu_potts_pop* P) {
    void* bufs[] = {P->d_pool, P->d_s, P->d_dis, P->d_part, P->d_ipart, P->d_E, P->d_neq, P->d_N,
                    P->d_W,    P->d_parent, P->d_xs, P->d_dead, P->d_pairs, P->d_npairs};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    ppop_free_history(P);
    delete P;
}

PopWalkers ppop_walkers(const tsu_potts_pop* P) { return PopWalkers{P->stride, (unsigned long long)P->seed, P->R}; }

// n_sweeps sweeps of every walker at T from the shared counter, on the plan's route
template <int DIM, bool HAS_H>
void ppop_enqueue_sweeps(tsu_potts_pop* P, const PottsPopPlan& pl, double T, int n_sweeps) {
    if (n_sweeps == 0) return;
    hipStream_t st = P->ctx->stream;
    PdSweep<DIM> p;
    p.s = P->d_pool;
    p.g = P->g;
    p.k = PottsKeys{0u, 0u, TSU_TAG_ISING_HI, TSU_TAG_ISING_LO};  // replica 0; the kernel fills in the walker's key
    p.m = P->m;
    p.m.T = T;
    const PopWalkers w = ppop_walkers(P);
    const uint32_t sweep0 = P->offset + P->sweeps;  // 32-bit words, as K12's
    p.hs = sweep0;
    if (pl.route == kPopRoutePack) {
        const unsigned groups = (unsigned)((P->R + pl.G - 1) / pl.G);
        hipLaunchKernelGGL((k14_pop_pack<DIM, HAS_H>), dim3(groups), dim3((unsigned)pl.threads), (size_t)pl.lds_bytes, st, p, w, pl.G, n_sweeps);
        P->launches += 1;
    } else if (pl.route == kPopRouteSmall) {
        hipLaunchKernelGGL((k14_pop_small<DIM, HAS_H>), dim3((unsigned)P->R), dim3((unsigned)pl.threads), 0, st, p, w, n_sweeps);
        P->launches += 1;
    } else {
        const dim3 grid((unsigned)((P->lanes + 255) / 256), (unsigned)P->R);
        for (int k = 0; k < n_sweeps; ++k)
            for (uint32_t colour = 0; colour < 2; ++colour) {
                p.hs = 2u * (sweep0 + (uint32_t)k) + colour;
                if ((P->g.cols & 15) == 0) hipLaunchKernelGGL((k14_pop_sweep<DIM, true, HAS_H>), grid, dim3(256), 0, st, p, w);
                else hipLaunchKernelGGL((k14_pop_sweep<DIM, false, HAS_H>), grid, dim3(256), 0, st, p, w);
                P->launches += 1;
            }
    }
    P->sweeps += (uint32_t)n_sweeps;
}

void ppop_sweeps(tsu_potts_pop* P, const PottsPopPlan& pl, double T, int n_sweeps) {
    if (P->dim == 2) {
        if (P->have_field) ppop_enqueue_sweeps<2, true>(P, pl, T, n_sweeps);
        else ppop_enqueue_sweeps<2, false>(P, pl, T, n_sweeps);
    } else {
        if (P->have_field) ppop_enqueue_sweeps<3, true>(P, pl, T, n_sweeps);
        else ppop_enqueue_sweeps<3, false>(P, pl, T, n_sweeps);
    }
}

// E, n_eq and N_c of every walker into E, n_eq, N (a history row or d_E, d_neq, d_N): two launches
void ppop_enqueue_measure(tsu_potts_pop* P, double* E, long long* n_eq, long long* N) {
    hipStream_t st = P->ctx->stream;
    PtpMeasure m = {P->d_pool, P->g, P->m, P->d_part, P->d_ipart};
    const dim3 grid(P->blocks, (unsigned)P->R);
    if (P->dim == 2) {
        if (P->have_field) hipLaunchKernelGGL((k14_pop_measure<2, true>), grid, dim3(256), 0, st, m, P->stride);
        else hipLaunchKernelGGL((k14_pop_measure<2, false>), grid, dim3(256), 0, st, m, P->stride);
    } else {
        if (P->have_field) hipLaunchKernelGGL((k14_pop_measure<3, true>), grid, dim3(256), 0, st, m, P->stride);
        else hipLaunchKernelGGL((k14_pop_measure<3, false>), grid, dim3(256), 0, st, m, P->stride);
    }
    hipLaunchKernelGGL(k13_pt_final, dim3((unsigned)P->R), dim3(256), 0, st, P->d_part, P->d_ipart, (int)P->blocks, E, n_eq, N);
    P->launches += 2;
}

int ppop_grow_history(tsu_potts_pop* P, size_t n) {
    tsu_ctx* ctx = P->ctx;
    if (P->hist_cap >= n && P->d_hE) return TSU_OK;
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // no kernel still writes the rows
    ppop_free_history(P);
    const size_t cap = n ? n : 1, R = (size_t)P->R;
    hipError_t e = hipMalloc((void**)&P->d_hE, (cap + 1) * R * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&P->d_hM, (cap + 1) * R * sizeof(long long));
    if (e == hipSuccess) e = hipMalloc((void**)&P->d_hN, (cap + 1) * R * TSU_POTTS_MAX_Q * sizeof(long long));
    if (e == hipSuccess) e = hipMalloc((void**)&P->d_hW, cap * R * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&P->d_hP, cap * R * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&P->d_hS, cap * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void**)&P->d_hU, cap * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void**)&P->d_hEmin, cap * sizeof(double));
    if (e != hipSuccess) {  // nothing of a history that does not fit stays behind
        ppop_free_history(P);
        (void)hipGetLastError();
        return tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "potts_pop_run: history of %zu steps: %s", n, hipGetErrorString(e));
    }
    P->hist_cap = cap;
    return TSU_OK;
}

int ppop_check_walker(tsu_potts_pop* P, const char* who, int i, const void* buf) {
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, buf, "potts_pop_%s: colours is NULL", who);
    TSU_REQUIRE(ctx, i >= 0 && i < P->R, "potts_pop_%s: walker %d out of range (population %d)", who, i, P->R);
    return TSU_OK;
}

}  // namespace

extern "C" {

int tsu_potts_pop_create(tsu_ctx* ctx, int depth, int rows, int cols, int q, const int* periodic, int population, tsu_potts_pop** out) {
    TSU_ENTER(ctx);
    if (!ctx || !out) return TSU_E_INVALID;
    *out = nullptr;
    TSU_REQUIRE(ctx, periodic, "potts_pop_create: periodic is NULL");
    const int pz = periodic[0] != 0, pr = periodic[1] != 0, pc = periodic[2] != 0;
    TSU_REQUIRE(ctx, q >= 2 && q <= TSU_POTTS_MAX_Q, "potts_pop_create: q must be in 2 .. 8 (got %d)", q);
    TSU_REQUIRE(ctx, depth >= 1 && rows >= 1 && cols >= 1, "potts_pop_create: depth, rows and cols must be >= 1");
    TSU_REQUIRE(ctx, (long long)depth * rows < (1ll << 31) && (long long)depth * rows * cols < (1ll << 31),
                "potts_pop_create: %lld x %d sites exceed 32-bit labels", (long long)depth * rows, cols);
    TSU_REQUIRE(ctx, (!pz || (depth & 1) == 0) && (!pr || (rows & 1) == 0) && (!pc || (cols & 1) == 0),
                "potts_pop_create: a periodic axis needs an even length");
    TSU_REQUIRE(ctx, population >= 2 && population <= kPopMaxWalkers, "potts_pop_create: population must be in [2, %d], got %d", kPopMaxWalkers,
                population);
    tsu_potts_pop* P = new (std::nothrow) tsu_potts_pop();
    if (!P) return tsu_fail(ctx, TSU_E_NOMEM, "potts_pop_create: host allocation failed");
    P->ctx = ctx;
    P->g = PottsGeom{depth, pz, pc, rows, cols, pr};
    P->dim = depth == 1 && !pz ? 2 : 3;
    P->q = q;
    P->R = population;
    P->sites = (long long)depth * rows * cols;
    P->stride = potts_pop_stride(P->sites);
    P->lanes = (long long)depth * rows * ((cols + 15) >> 4);
    P->m.q = q;
    P->m.sites = P->sites;
    P->blocks = reduce_blocks(P->sites);
    P->hist_steps = -1;
    const size_t R = (size_t)population, n = (size_t)P->sites;
    hipError_t e = hipSuccess;
    auto alloc = [&e](auto*& ptr, size_t bytes) {
        if (e == hipSuccess) e = hipMalloc((void**)&ptr, bytes);
    };
    alloc(P->d_pool, R * (size_t)P->stride);
    alloc(P->d_s, R * sizeof(int8_t*));
    alloc(P->d_dis, (size_t)((P->dim == 2 ? 2 : 3) + q) * n * sizeof(float));
    alloc(P->d_part, R * P->blocks * sizeof(double));
    alloc(P->d_ipart, R * P->blocks * TSU_POTTS_RECORD_WORDS * sizeof(unsigned long long));
    alloc(P->d_E, R * sizeof(double));
    alloc(P->d_neq, R * sizeof(long long));
    alloc(P->d_N, R * TSU_POTTS_MAX_Q * sizeof(long long));
    alloc(P->d_W, R * sizeof(uint32_t));
    alloc(P->d_parent, R * sizeof(int32_t));
    alloc(P->d_xs, (R + 1) * sizeof(uint32_t));
    alloc(P->d_dead, R * sizeof(int32_t));
    alloc(P->d_pairs, R * sizeof(int2));
    alloc(P->d_npairs, sizeof(uint32_t));
    std::vector<int8_t*> planes(R);
    if (e == hipSuccess)
        for (size_t i = 0; i < R; ++i) planes[i] = P->d_pool + i * (size_t)P->stride;
    if (e == hipSuccess) e = hipMemsetAsync(P->d_pool, 0, R * (size_t)P->stride, ctx->stream);  // the pad bytes stay 0
    if (e == hipSuccess) e = hipMemcpyAsync(P->d_s, planes.data(), R * sizeof(int8_t*), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(P->d_npairs, 0, sizeof(uint32_t), ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // before `planes` goes
    if (e != hipSuccess) {  // a population that does not fit leaves nothing behind, HIP's last error included
        const int rc = tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "potts_pop_create: population of %d lattices of %zu bytes: %s",
                                population, n, hipGetErrorString(e));
        (void)hipStreamSynchronize(ctx->stream);
        ppop_free(P);
        (void)hipGetLastError();
        return rc;
    }
    *out = P;
    return TSU_OK;
}

int tsu_potts_pop_destroy(tsu_potts_pop* P) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    (void)hipStreamSynchronize(P->ctx->stream);
    ppop_free(P);
    return TSU_OK;
}

int tsu_potts_pop_set_disorder(tsu_potts_pop* P, const float* J_right, const float* J_down, const float* J_layer, const float* h) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, J_right && J_down, "potts_pop_set_disorder: J_right and J_down are required");
    // a 2-D lattice given with a J_layer holds the open z axis's only layer, which must be 0 as on any open axis; it is not stored
    TSU_REQUIRE(ctx, P->dim == 2 || J_layer, "potts_pop_set_disorder: a 3-D lattice needs J_layer");
    const int depth = P->g.depth, rows = P->g.rows, cols = P->g.cols;
    const size_t n = (size_t)P->sites;
    for (int z = 0; z < depth; ++z)
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) {
                const size_t i = ((size_t)z * rows + r) * cols + c;
                const float jl = J_layer ? J_layer[i] : 0.0f;
                TSU_REQUIRE(ctx, isfinite(J_right[i]) && isfinite(J_down[i]) && isfinite(jl),
                            "potts_pop_set_disorder: non-finite coupling at site (%d, %d, %d)", z, r, c);
                TSU_REQUIRE(ctx, P->g.pc || c + 1 < cols || J_right[i] == 0.0f,
                            "potts_pop_set_disorder: open axis: J_right[%d, %d, %d] (last column) must be 0, got %g", z, r, c, (double)J_right[i]);
                TSU_REQUIRE(ctx, P->g.pr || r + 1 < rows || J_down[i] == 0.0f,
                            "potts_pop_set_disorder: open axis: J_down[%d, %d, %d] (last row) must be 0, got %g", z, r, c, (double)J_down[i]);
                TSU_REQUIRE(ctx, P->g.pz || z + 1 < depth || jl == 0.0f,
                            "potts_pop_set_disorder: open axis: J_layer[%d, %d, %d] (last layer) must be 0, got %g", z, r, c, (double)jl);
            }
    if (h)
        for (size_t i = 0; i < n * (size_t)P->q; ++i)
            TSU_REQUIRE(ctx, isfinite(h[i]), "potts_pop_set_disorder: non-finite field at colour %zu, site %zu", i / n, i % n);
    const int nj = P->dim == 2 ? 2 : 3;
    const float* src[3] = {J_right, J_down, J_layer};
    for (int k = 0; k < nj; ++k)
        TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_dis + (size_t)k * n, src[k], n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    if (h) TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_dis + (size_t)nj * n, h, (size_t)P->q * n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    P->m.jr = P->d_dis;
    P->m.jd = P->d_dis + n;
    P->m.jl = P->dim == 2 ? nullptr : P->d_dis + 2 * n;
    P->m.h = h ? P->d_dis + (size_t)nj * n : nullptr;
    P->have_disorder = 1;
    P->have_field = h != nullptr;
    P->have_E = 0;
    return TSU_OK;
}

int tsu_potts_pop_set_schedule(tsu_potts_pop* P, const double* betas, int n) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, betas, "potts_pop_set_schedule: NULL betas");
    TSU_REQUIRE(ctx, n >= 2 && n - 1 <= kPottsPopMaxSteps, "potts_pop_set_schedule: need 2 to %d inverse temperatures, got %d", kPottsPopMaxSteps + 1,
                n);
    TSU_REQUIRE(ctx, betas[0] >= 0.0 && isfinite(betas[0]), "potts_pop_set_schedule: beta[0] must be finite and >= 0, got %g", betas[0]);
    for (int k = 1; k < n; ++k)
        TSU_REQUIRE(ctx, isfinite(betas[k]) && betas[k] > betas[k - 1], "potts_pop_set_schedule: betas must increase (beta[%d] = %g after %g)", k,
                    betas[k], betas[k - 1]);
    P->beta.assign(betas, betas + n);
    P->K = n - 1;
    P->have_sched = 1;
    P->have_init = 0;
    P->step = 0;
    return TSU_OK;
}

int tsu_potts_pop_init(tsu_potts_pop* P, uint64_t seed, int initial, int initial_sweeps) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, P->have_disorder, "potts_pop_init: call tsu_potts_pop_set_disorder first");
    TSU_REQUIRE(ctx, P->have_sched, "potts_pop_init: call tsu_potts_pop_set_schedule first");
    TSU_REQUIRE(ctx, initial >= -2 && initial < P->q,
                "potts_pop_init: initial must be -2 (the device draw), -1 (keep the colours) or a colour in 0 .. %d, got %d", P->q - 1, initial);
    TSU_REQUIRE(ctx, initial_sweeps >= 0, "potts_pop_init: initial_sweeps must be >= 0, got %d", initial_sweeps);
    P->have_init = 0;
    P->seed = seed;
    P->sweeps = 0;
    P->offset = 0;
    P->step = 0;
    P->hist_steps = -1;
    if (initial >= 0) {  // walker by walker: the pad bytes stay 0
        TSU_HIP_TRY(ctx, hipMemset2DAsync(P->d_pool, (size_t)P->stride, initial, (size_t)P->sites, (size_t)P->R, ctx->stream));
    } else if (initial == -2) {
        hipLaunchKernelGGL(k14_pop_init, dim3((unsigned)((P->lanes + 255) / 256), (unsigned)P->R), dim3(256), 0, ctx->stream, P->d_pool,
                           ppop_walkers(P), P->g.depth * P->g.rows, P->g.cols, P->q);
        P->launches += 1;
    }
    if (P->beta[0] > 0.0) ppop_sweeps(P, ppop_plan(P), 1.0 / P->beta[0], initial_sweeps);
    ppop_enqueue_measure(P, P->d_E, P->d_neq, P->d_N);
    TSU_HIP_TRY(ctx, hipGetLastError());
    P->have_E = 1;
    P->have_init = 1;
    return TSU_OK;
}

int tsu_potts_pop_advance(tsu_potts_pop* P, uint64_t n_sweeps) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    TSU_REQUIRE(P->ctx, P->have_init, "potts_pop_advance: call tsu_potts_pop_init first");
    P->offset += (uint32_t)n_sweeps;
    return TSU_OK;
}

int tsu_potts_pop_run(tsu_potts_pop* P, int n_steps, int sweeps_per_step, int resample, int record) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, P->have_disorder, "potts_pop_run: call tsu_potts_pop_set_disorder first");
    TSU_REQUIRE(ctx, P->have_sched, "potts_pop_run: call tsu_potts_pop_set_schedule first");
    TSU_REQUIRE(ctx, P->have_init, "potts_pop_run: call tsu_potts_pop_init first");
    TSU_REQUIRE(ctx, n_steps >= 0 && sweeps_per_step >= 0, "potts_pop_run: need n_steps >= 0 and sweeps_per_step >= 0 (got %d, %d)", n_steps,
                sweeps_per_step);
    TSU_REQUIRE(ctx, (uint64_t)P->step + (uint64_t)n_steps <= (uint64_t)P->K, "potts_pop_run: %d steps from step %u run past the schedule of %d steps",
                n_steps, P->step, P->K);
    TSU_REQUIRE(ctx, (uint64_t)P->sweeps + (uint64_t)n_steps * (uint64_t)sweeps_per_step <= (1ull << 31), "potts_pop_run: sweep counter overflow");
    const size_t R = (size_t)P->R, n = (size_t)n_steps;
    hipStream_t st = ctx->stream;
    if (record) {
        const int rc = ppop_grow_history(P, n);
        if (rc != TSU_OK) return rc;
    }
    P->hist_steps = record ? n_steps : -1;
    if (!P->have_E) {  // the colours or the disorder changed since the last pass
        ppop_enqueue_measure(P, P->d_E, P->d_neq, P->d_N);
        P->have_E = 1;
    }
    if (record) {
        TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_hE, P->d_E, R * sizeof(double), hipMemcpyDeviceToDevice, st));
        TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_hM, P->d_neq, R * sizeof(long long), hipMemcpyDeviceToDevice, st));
        TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_hN, P->d_N, R * TSU_POTTS_MAX_Q * sizeof(long long), hipMemcpyDeviceToDevice, st));
        if (!resample && n) {
            const size_t nb = (n * R + 255) / 256;
            hipLaunchKernelGGL(pop_identity, dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(256), 0, st, P->d_hP, P->R, (long long)(n * R));
            P->launches += 1;
            TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_hW, 0, n * R * sizeof(uint32_t), st));
            TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_hS, 0, n * sizeof(unsigned long long), st));
            TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_hU, 0, n * sizeof(unsigned long long), st));
            TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_hEmin, 0, n * sizeof(double), st));
        }
    }
    const PottsPopPlan route = ppop_plan(P);
    PopPlan pl;
    pl.xs = P->d_xs;
    pl.dead = P->d_dead;
    pl.pairs = P->d_pairs;
    pl.n_pairs = P->d_npairs;
    pl.R = P->R;
    pl.k0 = (uint32_t)P->seed;
    pl.k1 = (uint32_t)(P->seed >> 32);
    const uint32_t cpp = (uint32_t)(P->stride / 16);  // create: stride < 2^31 + 16
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
            hipLaunchKernelGGL(pop_plan, dim3(1), dim3(kPopPlanThreads), 0, st, pl);
            hipLaunchKernelGGL(pop_copy, dim3(copy_grid), dim3(256), 0, st, P->d_s, P->d_pairs, P->d_npairs, cpp);
            P->launches += 2;
        }
        ppop_sweeps(P, route, 1.0 / P->beta[k], sweeps_per_step);
        double* E = record ? P->d_hE + (j + 1) * R : P->d_E;  // the measuring pass writes straight into the history rows
        ppop_enqueue_measure(P, E, record ? P->d_hM + (j + 1) * R : P->d_neq, record ? P->d_hN + (j + 1) * R * TSU_POTTS_MAX_Q : P->d_N);
        curE = E;
        P->step += 1;
    }
    if (record && n) {  // between runs the current energies live in d_E, d_neq, d_N
        TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_E, P->d_hE + n * R, R * sizeof(double), hipMemcpyDeviceToDevice, st));
        TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_neq, P->d_hM + n * R, R * sizeof(long long), hipMemcpyDeviceToDevice, st));
        TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_N, P->d_hN + n * R * TSU_POTTS_MAX_Q, R * TSU_POTTS_MAX_Q * sizeof(long long), hipMemcpyDeviceToDevice, st));
    }
    TSU_HIP_TRY(ctx, hipGetLastError());  // one check for all the launches above
    return TSU_OK;
}

int tsu_potts_pop_history(tsu_potts_pop* P, double* E, int64_t* n_eq, int64_t* N, uint32_t* W, int32_t* parent, uint64_t* S, uint64_t* U,
                          double* E_min) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, P->hist_steps >= 0 && P->d_hE, "potts_pop_history: the last run recorded nothing");
    const size_t n = (size_t)P->hist_steps, R = (size_t)P->R;
    hipStream_t st = ctx->stream;
    if (E) TSU_HIP_TRY(ctx, hipMemcpyAsync(E, P->d_hE, (n + 1) * R * sizeof(double), hipMemcpyDeviceToHost, st));
    if (n_eq) TSU_HIP_TRY(ctx, hipMemcpyAsync(n_eq, P->d_hM, (n + 1) * R * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (N) TSU_HIP_TRY(ctx, hipMemcpyAsync(N, P->d_hN, (n + 1) * R * TSU_POTTS_MAX_Q * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (n) {
        if (W) TSU_HIP_TRY(ctx, hipMemcpyAsync(W, P->d_hW, n * R * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (parent) TSU_HIP_TRY(ctx, hipMemcpyAsync(parent, P->d_hP, n * R * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (S) TSU_HIP_TRY(ctx, hipMemcpyAsync(S, P->d_hS, n * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        if (U) TSU_HIP_TRY(ctx, hipMemcpyAsync(U, P->d_hU, n * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        if (E_min) TSU_HIP_TRY(ctx, hipMemcpyAsync(E_min, P->d_hEmin, n * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    TSU_HIP_TRY(ctx, hipStreamSynchronize(st));
    return TSU_OK;
}

int tsu_potts_pop_energies(tsu_potts_pop* P, double* E, int64_t* n_eq) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, P->have_disorder, "potts_pop_energies: call tsu_potts_pop_set_disorder first");
    TSU_REQUIRE(ctx, P->have_init, "potts_pop_energies: call tsu_potts_pop_init first");
    ppop_enqueue_measure(P, P->d_E, P->d_neq, P->d_N);
    TSU_HIP_TRY(ctx, hipGetLastError());
    P->have_E = 1;
    const size_t R = (size_t)P->R;
    if (E) TSU_HIP_TRY(ctx, hipMemcpyAsync(E, P->d_E, R * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (n_eq) TSU_HIP_TRY(ctx, hipMemcpyAsync(n_eq, P->d_neq, R * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int tsu_potts_pop_get_spins(tsu_potts_pop* P, int i, int8_t* colours) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    const int rc = ppop_check_walker(P, "get_spins", i, colours);
    if (rc != TSU_OK) return rc;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(colours, P->d_pool + (size_t)i * (size_t)P->stride, (size_t)P->sites, hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int tsu_potts_pop_set_spins(tsu_potts_pop* P, int i, const int8_t* colours) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    const int rc = ppop_check_walker(P, "set_spins", i, colours);
    if (rc != TSU_OK) return rc;
    const size_t n = (size_t)P->sites;
    for (size_t k = 0; k < n; ++k)
        TSU_REQUIRE(ctx, colours[k] >= 0 && colours[k] < P->q, "potts_pop_set_spins: colour %d at site %zu is outside 0 .. %d", (int)colours[k], k,
                    P->q - 1);
    TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_pool + (size_t)i * (size_t)P->stride, colours, n, hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    P->have_E = 0;
    return TSU_OK;
}

int tsu_potts_pop_get_padded(tsu_potts_pop* P, int i, int8_t* bytes) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    const int rc = ppop_check_walker(P, "get_padded", i, bytes);
    if (rc != TSU_OK) return rc;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(bytes, P->d_pool + (size_t)i * (size_t)P->stride, (size_t)P->stride, hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int tsu_potts_pop_route(tsu_potts_pop* P, int* route) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P || !route) return TSU_E_INVALID;
    *route = ppop_plan(P).route;
    return TSU_OK;
}

int tsu_potts_pop_plan(tsu_potts_pop* P, int* route, int* G, int* threads, int* lds_bytes) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const PottsPopPlan pl = ppop_plan(P);
    if (route) *route = pl.route;
    if (G) *G = pl.G;
    if (threads) *threads = pl.threads;
    if (lds_bytes) *lds_bytes = pl.lds_bytes;
    return TSU_OK;
}

int tsu_potts_pop_launch_count(tsu_potts_pop* P, uint64_t* n) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P || !n) return TSU_E_INVALID;
    *n = P->launches;
    return TSU_OK;
}

}  // extern "C"

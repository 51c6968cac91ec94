// potts_pt.hip -- K13: parallel tempering of K12's Potts lattice (gfx950), the host side and the C ABI of
// include/tsu_hip_potts_pt.h; the contract is DESIGN.md section 3, "Parallel tempering (K13)".  The kernels are
// potts_pt_kern_dev.h's, which run K12's octet bodies and measuring order per walker; the swap pass is the ladders' own k7_pt_swap
// (pt_dev.h), filled through a PTSwap from this handle's tables as sparse_batch.hip does.  One handle serves both dimensions, as
// K12's does: depth 1 with an open z axis launches the DIM = 2 instantiations.
#include <math.h>
#include <stdlib.h>

#include <vector>

#include "potts_pt_kern_dev.h"
#include "pt_host.h"  // pt_enqueue_swap: the one launch of the swap pass
#include "sw_host.h"  // sw_threads: k12_small's lanes

struct tsu_potts_pt {
    tsu_ctx* ctx;
    PottsGeom g;  // 2-D: depth 1, pz 0
    int dim, q, R, nl, nw;
    long long sites;
    int8_t* d_s;   // nw lattices of `sites` colours, walker g at d_s + g sites: one allocation
    float* d_dis;  // J_right, J_down, J_layer (3-D), then the q colour planes of h (when given): one copy for all walkers
    PdModel m;
    int have_disorder, have_field, have_T, have_init;
    uint64_t sweeps;  // sweeps of every walker since init; the kernels get its low word
    uint32_t rounds;
    unsigned long long launches;
    unsigned blocks;  // pd_measure_blocks of the shape
    uint32_t* d_key;  // walker -> (k0, k1)
    int32_t *d_slot, *d_was, *d_flag;
    double* d_T;
    long long *d_att, *d_acc, *d_trips;
    double* d_part;             // [walker][blocks]
    unsigned long long* d_ipart;  // [walker][blocks][9]
    double* d_E;                // walker -> E of the last measuring pass
    long long *d_neq, *d_N;     // walker -> n_eq; [walker][8] colour counts
    double* d_hE;               // [round][ladder][slot]
    long long *d_hM, *d_hN, *d_hC;  // n_eq [round][ladder][slot]; N [..][8]; tables [round][slot][q q]
    int32_t* d_hW;
    size_t hist_cap;
    int hist_rounds;
    uint32_t key0, key1;  // the swap uniforms' key: the seed
};

namespace {

bool ptp_small_switch_off() {  // TSU_POTTS_SMALL=0 (tests, read per call): every lattice on k13_pt_sweep
    const char* e = getenv("TSU_POTTS_SMALL");
    return e && atoi(e) == 0;
}

bool ptp_small_route(const tsu_potts_pt* P) { return !ptp_small_switch_off() && P->sites <= kPottsSmallSites; }

void ptp_free_history(tsu_potts_pt* P) {
    void* bufs[] = {P->d_hE, P->d_hM, P->d_hN, P->d_hC, P->d_hW};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    P->d_hE = nullptr;
    P->d_hM = P->d_hN = P->d_hC = nullptr;
    P->d_hW = nullptr;
    P->hist_cap = 0;
    P->hist_rounds = 0;
}

void ptp_free(tsu_potts_pt* P) {
    void* bufs[] = {P->d_s,   P->d_dis,  P->d_key,   P->d_slot, P->d_was, P->d_flag, P->d_T,  P->d_att,
                    P->d_acc, P->d_trips, P->d_part, P->d_ipart, P->d_E,  P->d_neq,  P->d_N};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    ptp_free_history(P);
    delete P;
}

// every walker at its own slot, the walker at slot 0 "bottom", no attempts, accepts or round trips (synchronises)
int ptp_reset(tsu_potts_pt* P) {
    tsu_ctx* ctx = P->ctx;
    const int R = P->R, nl = P->nl;
    std::vector<int32_t> ident((size_t)P->nw), flag((size_t)P->nw, kPtNone);
    for (int k = 0; k < nl; ++k) {
        for (int w = 0; w < R; ++w) ident[(size_t)k * R + w] = w;
        flag[(size_t)k * R] = kPtBottom;
    }
    const size_t b = (size_t)P->nw * sizeof(int32_t);
    TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_slot, ident.data(), b, hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_was, ident.data(), b, hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_flag, flag.data(), b, hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_att, 0, (size_t)nl * (R - 1) * sizeof(long long), ctx->stream));
    TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_acc, 0, (size_t)nl * (R - 1) * sizeof(long long), ctx->stream));
    TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_trips, 0, (size_t)P->nw * sizeof(long long), ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    P->sweeps = 0;
    P->rounds = 0;
    P->hist_rounds = 0;
    return TSU_OK;
}

int ptp_check_slot(tsu_potts_pt* P, const char* who, int ladder, int slot, int32_t* walker) {
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, ladder >= 0 && ladder < P->nl && slot >= 0 && slot < P->R, "potts_pt_%s: (ladder %d, slot %d) is outside %d x %d", who, ladder,
                slot, P->nl, P->R);
    TSU_HIP_TRY(ctx, hipMemcpyAsync(walker, P->d_was + (size_t)ladder * P->R + slot, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

template <int DIM>
PdSweep<DIM> ptp_sweep_params(const tsu_potts_pt* P) {
    PdSweep<DIM> p;
    p.s = P->d_s;
    p.g = P->g;
    p.k = PottsKeys{0u, 0u, TSU_TAG_ISING_HI, TSU_TAG_ISING_LO};  // replica 0; the kernel fills in the walker's key
    p.hs = 0;
    p.m = P->m;
    p.m.T = 0.0;  // the kernel reads the slot's
    return p;
}

// swap_interval sweeps of every walker from sweep counter P->sweeps
template <int DIM, bool HAS_H>
void ptp_enqueue_sweeps(tsu_potts_pt* P, int n_sweeps, bool small) {
    hipStream_t st = P->ctx->stream;
    PdSweep<DIM> p = ptp_sweep_params<DIM>(P);
    const PtpTables t = {P->d_key, P->d_slot, P->d_T};
    const uint32_t sweep0 = (uint32_t)P->sweeps;
    const long long lanes = (long long)P->g.depth * P->g.rows * ((P->g.cols + 15) >> 4);
    if (small) {
        p.hs = sweep0;
        hipLaunchKernelGGL((k13_pt_small<DIM, HAS_H>), dim3((unsigned)P->nw), dim3((unsigned)sw_threads(lanes)), 0, st, p, t, n_sweeps);
        P->launches += 1;
        return;
    }
    const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)P->nw);
    for (int k = 0; k < n_sweeps; ++k)
        for (uint32_t colour = 0; colour < 2; ++colour) {
            p.hs = 2u * (sweep0 + (uint32_t)k) + colour;  // 32-bit words, as K12's
            if ((P->g.cols & 15) == 0) hipLaunchKernelGGL((k13_pt_sweep<DIM, true, HAS_H>), grid, dim3(256), 0, st, p, t);
            else hipLaunchKernelGGL((k13_pt_sweep<DIM, false, HAS_H>), grid, dim3(256), 0, st, p, t);
            P->launches += 1;
        }
}

void ptp_sweeps(tsu_potts_pt* P, int n_sweeps, bool small) {
    if (P->dim == 2) {
        if (P->have_field) ptp_enqueue_sweeps<2, true>(P, n_sweeps, small);
        else ptp_enqueue_sweeps<2, false>(P, n_sweeps, small);
    } else {
        if (P->have_field) ptp_enqueue_sweeps<3, true>(P, n_sweeps, small);
        else ptp_enqueue_sweeps<3, false>(P, n_sweeps, small);
    }
}

// E, n_eq and N_c of every walker into d_E, d_neq, d_N: two launches
void ptp_enqueue_measure(tsu_potts_pt* P) {
    hipStream_t st = P->ctx->stream;
    PtpMeasure m = {P->d_s, P->g, P->m, P->d_part, P->d_ipart};
    const dim3 grid(P->blocks, (unsigned)P->nw);
    if (P->dim == 2) {
        if (P->have_field) hipLaunchKernelGGL((k13_pt_measure<2, true>), grid, dim3(256), 0, st, m);
        else hipLaunchKernelGGL((k13_pt_measure<2, false>), grid, dim3(256), 0, st, m);
    } else {
        if (P->have_field) hipLaunchKernelGGL((k13_pt_measure<3, true>), grid, dim3(256), 0, st, m);
        else hipLaunchKernelGGL((k13_pt_measure<3, false>), grid, dim3(256), 0, st, m);
    }
    hipLaunchKernelGGL(k13_pt_final, dim3((unsigned)P->nw), dim3(256), 0, st, P->d_part, P->d_ipart, (int)P->blocks, P->d_E, P->d_neq, P->d_N);
    P->launches += 2;
}

int ptp_grow_history(tsu_potts_pt* P, int n_rounds) {
    tsu_ctx* ctx = P->ctx;
    if (P->hist_cap >= (size_t)n_rounds) return TSU_OK;
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // no kernel still writes the rows
    ptp_free_history(P);
    const size_t rows = (size_t)n_rounds * P->nw;
    hipError_t e = hipMalloc((void**)&P->d_hE, rows * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&P->d_hM, rows * sizeof(long long));
    if (e == hipSuccess) e = hipMalloc((void**)&P->d_hN, rows * TSU_POTTS_MAX_Q * sizeof(long long));
    if (e == hipSuccess) e = hipMalloc((void**)&P->d_hW, rows * sizeof(int32_t));
    if (e == hipSuccess && P->nl == 2) e = hipMalloc((void**)&P->d_hC, (size_t)n_rounds * P->R * P->q * P->q * sizeof(long long));
    if (e != hipSuccess) {
        ptp_free_history(P);
        (void)hipGetLastError();
        return tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "potts_pt_run: history of %d rounds: %s", n_rounds,
                        hipGetErrorString(e));
    }
    P->hist_cap = (size_t)n_rounds;
    return TSU_OK;
}

}  // namespace

extern "C" {

int tsu_potts_pt_create(tsu_ctx* ctx, int depth, int rows, int cols, int q, const int* periodic, int n_temps, int n_ladders,
                        tsu_potts_pt** out) {
    TSU_ENTER(ctx);
    if (!ctx || !out) return TSU_E_INVALID;
    *out = nullptr;
    TSU_REQUIRE(ctx, periodic, "potts_pt_create: periodic is NULL");
    const int pz = periodic[0] != 0, pr = periodic[1] != 0, pc = periodic[2] != 0;
    TSU_REQUIRE(ctx, q >= 2 && q <= TSU_POTTS_MAX_Q, "potts_pt_create: q must be in 2 .. 8 (got %d)", q);
    TSU_REQUIRE(ctx, depth >= 1 && rows >= 1 && cols >= 1, "potts_pt_create: depth, rows and cols must be >= 1");
    TSU_REQUIRE(ctx, (long long)depth * rows < (1ll << 31) && (long long)depth * rows * cols < (1ll << 31),
                "potts_pt_create: %lld x %d sites exceed 32-bit labels", (long long)depth * rows, cols);
    TSU_REQUIRE(ctx, (!pz || (depth & 1) == 0) && (!pr || (rows & 1) == 0) && (!pc || (cols & 1) == 0),
                "potts_pt_create: a periodic axis needs an even length");
    TSU_REQUIRE(ctx, n_temps >= 2 && n_temps <= kPtMaxTemps, "potts_pt_create: n_temps must be in [2, %d], got %d", kPtMaxTemps, n_temps);
    TSU_REQUIRE(ctx, n_ladders == 1 || n_ladders == 2, "potts_pt_create: n_ladders must be 1 or 2, got %d", n_ladders);
    tsu_potts_pt* P = new (std::nothrow) tsu_potts_pt();
    if (!P) return tsu_fail(ctx, TSU_E_NOMEM, "potts_pt_create: host allocation failed");
    P->ctx = ctx;
    P->g = PottsGeom{depth, pz, pc, rows, cols, pr};
    P->dim = depth == 1 && !pz ? 2 : 3;
    P->q = q;
    P->R = n_temps;
    P->nl = n_ladders;
    P->nw = n_temps * n_ladders;
    P->sites = (long long)depth * rows * cols;
    P->m.q = q;
    P->m.sites = P->sites;
    P->blocks = reduce_blocks(P->sites);
    const size_t nw = (size_t)P->nw, n = (size_t)P->sites, R = (size_t)n_temps, nl = (size_t)n_ladders;
    hipError_t e = hipSuccess;
    auto alloc = [&e](auto*& ptr, size_t bytes) {
        if (e == hipSuccess) e = hipMalloc((void**)&ptr, bytes);
    };
    alloc(P->d_s, nw * n);
    alloc(P->d_dis, (size_t)((P->dim == 2 ? 2 : 3) + q) * n * sizeof(float));
    alloc(P->d_key, 2 * nw * sizeof(uint32_t));
    alloc(P->d_slot, nw * sizeof(int32_t));
    alloc(P->d_was, nw * sizeof(int32_t));
    alloc(P->d_flag, nw * sizeof(int32_t));
    alloc(P->d_T, R * sizeof(double));
    alloc(P->d_att, nl * (R - 1) * sizeof(long long));
    alloc(P->d_acc, nl * (R - 1) * sizeof(long long));
    alloc(P->d_trips, nw * sizeof(long long));
    alloc(P->d_part, nw * P->blocks * sizeof(double));
    alloc(P->d_ipart, nw * P->blocks * TSU_POTTS_RECORD_WORDS * sizeof(unsigned long long));
    alloc(P->d_E, nw * sizeof(double));
    alloc(P->d_neq, nw * sizeof(long long));
    alloc(P->d_N, nw * TSU_POTTS_MAX_Q * sizeof(long long));
    if (e == hipSuccess) e = hipMemsetAsync(P->d_s, 0, nw * n, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(P->d_key, 0, 2 * nw * sizeof(uint32_t), ctx->stream);
    int rc = TSU_OK;
    if (e != hipSuccess) {
        rc = tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "potts_pt_create: %d lattices of %zu bytes: %s", P->nw, n,
                      hipGetErrorString(e));
        (void)hipStreamSynchronize(ctx->stream);
    } else {
        rc = ptp_reset(P);
    }
    if (rc != TSU_OK) {  // a ladder that does not fit leaves nothing behind, HIP's last error included
        ptp_free(P);
        (void)hipGetLastError();
        return rc;
    }
    *out = P;
    return TSU_OK;
}

int tsu_potts_pt_destroy(tsu_potts_pt* P) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    (void)hipStreamSynchronize(P->ctx->stream);
    ptp_free(P);
    return TSU_OK;
}

int tsu_potts_pt_set_disorder(tsu_potts_pt* P, const float* J_right, const float* J_down, const float* J_layer, const float* h) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, J_right && J_down, "potts_pt_set_disorder: J_right and J_down are required");
    // a 2-D lattice given with a J_layer holds the open z axis's only layer, which must be 0 as on any open axis; it is not stored
    TSU_REQUIRE(ctx, P->dim == 2 || J_layer, "potts_pt_set_disorder: a 3-D lattice needs J_layer");
    const int depth = P->g.depth, rows = P->g.rows, cols = P->g.cols;
    const size_t n = (size_t)P->sites;
    for (int z = 0; z < depth; ++z)
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) {
                const size_t i = ((size_t)z * rows + r) * cols + c;
                const float jl = J_layer ? J_layer[i] : 0.0f;
                TSU_REQUIRE(ctx, isfinite(J_right[i]) && isfinite(J_down[i]) && isfinite(jl),
                            "potts_pt_set_disorder: non-finite coupling at site (%d, %d, %d)", z, r, c);
                TSU_REQUIRE(ctx, P->g.pc || c + 1 < cols || J_right[i] == 0.0f,
                            "potts_pt_set_disorder: open axis: J_right[%d, %d, %d] (last column) must be 0, got %g", z, r, c, (double)J_right[i]);
                TSU_REQUIRE(ctx, P->g.pr || r + 1 < rows || J_down[i] == 0.0f,
                            "potts_pt_set_disorder: open axis: J_down[%d, %d, %d] (last row) must be 0, got %g", z, r, c, (double)J_down[i]);
                TSU_REQUIRE(ctx, P->g.pz || z + 1 < depth || jl == 0.0f,
                            "potts_pt_set_disorder: open axis: J_layer[%d, %d, %d] (last layer) must be 0, got %g", z, r, c, (double)jl);
            }
    if (h)
        for (size_t i = 0; i < n * (size_t)P->q; ++i)
            TSU_REQUIRE(ctx, isfinite(h[i]), "potts_pt_set_disorder: non-finite field at colour %zu, site %zu", i / n, i % n);
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
    return TSU_OK;
}

int tsu_potts_pt_set_temperatures(tsu_potts_pt* P, const double* T) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, T, "potts_pt_set_temperatures: T is NULL");
    for (int i = 0; i < P->R; ++i) TSU_REQUIRE(ctx, isfinite(T[i]) && T[i] > 0.0, "Temperature must be positive (slot %d: %g)", i, T[i]);
    TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_T, T, (size_t)P->R * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    P->have_T = 1;
    return TSU_OK;
}

int tsu_potts_pt_set_spins(tsu_potts_pt* P, int ladder, int slot, const int8_t* colours) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, colours, "potts_pt_set_spins: colours is NULL");
    const size_t n = (size_t)P->sites;
    for (size_t i = 0; i < n; ++i)
        TSU_REQUIRE(ctx, colours[i] >= 0 && colours[i] < P->q, "potts_pt_set_spins: colour %d at site %zu is outside 0 .. %d", (int)colours[i], i,
                    P->q - 1);
    int32_t w = 0;
    const int rc = ptp_check_slot(P, "set_spins", ladder, slot, &w);
    if (rc != TSU_OK) return rc;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_s + ((size_t)ladder * P->R + w) * n, colours, n, hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int tsu_potts_pt_get_spins(tsu_potts_pt* P, int ladder, int slot, int8_t* colours) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, colours, "potts_pt_get_spins: colours is NULL");
    int32_t w = 0;
    const int rc = ptp_check_slot(P, "get_spins", ladder, slot, &w);
    if (rc != TSU_OK) return rc;
    const size_t n = (size_t)P->sites;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(colours, P->d_s + ((size_t)ladder * P->R + w) * n, n, hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int tsu_potts_pt_init(tsu_potts_pt* P, uint64_t seed, int initial) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, initial >= -1 && initial < P->q, "potts_pt_init: initial must be -1 (keep the colours) or a colour in 0 .. %d, got %d", P->q - 1,
                initial);
    std::vector<uint32_t> keys(2 * (size_t)P->nw);
    for (int g = 0; g < P->nw; ++g) {
        const uint64_t s = seed + (uint64_t)g;
        keys[2 * (size_t)g] = (uint32_t)s;
        keys[2 * (size_t)g + 1] = (uint32_t)(s >> 32);
    }
    TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_key, keys.data(), keys.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    if (initial >= 0) TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_s, initial, (size_t)P->nw * (size_t)P->sites, ctx->stream));
    const int rc = ptp_reset(P);  // synchronises before `keys` goes
    if (rc != TSU_OK) return rc;
    P->key0 = (uint32_t)seed;
    P->key1 = (uint32_t)(seed >> 32);
    P->have_init = 1;
    return TSU_OK;
}

int tsu_potts_pt_advance(tsu_potts_pt* P, uint64_t n_sweeps) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    TSU_REQUIRE(P->ctx, P->have_init, "potts_pt_advance: call tsu_potts_pt_init first");
    P->sweeps += n_sweeps;
    return TSU_OK;
}

int tsu_potts_pt_run(tsu_potts_pt* P, int n_rounds, int swap_interval, int do_swap, int record) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, P->have_disorder, "potts_pt_run: call tsu_potts_pt_set_disorder first");
    TSU_REQUIRE(ctx, P->have_T, "potts_pt_run: call tsu_potts_pt_set_temperatures first");
    TSU_REQUIRE(ctx, P->have_init, "potts_pt_run: call tsu_potts_pt_init first");
    TSU_REQUIRE(ctx, n_rounds >= 0 && swap_interval >= 1, "potts_pt_run: need n_rounds >= 0 and swap_interval >= 1 (got %d, %d)", n_rounds,
                swap_interval);
    TSU_REQUIRE(ctx, (uint64_t)n_rounds * (uint64_t)swap_interval <= (1ull << 31), "potts_pt_run: %llu sweeps exceed one call",
                (unsigned long long)n_rounds * (unsigned long long)swap_interval);
    TSU_REQUIRE(ctx, (uint64_t)P->rounds + (uint64_t)n_rounds <= 0xFFFFFFFFull, "potts_pt_run: round counter overflow");
    const int R = P->R, nl = P->nl, q = P->q;
    if (record) {
        const int rc = ptp_grow_history(P, n_rounds);
        if (rc != TSU_OK) return rc;
        if (nl == 2 && n_rounds > 0)  // k13_pt_table adds into its rows
            TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_hC, 0, (size_t)n_rounds * R * q * q * sizeof(long long), ctx->stream));
    }
    P->hist_rounds = record ? n_rounds : 0;
    const bool small = ptp_small_route(P);
    hipStream_t st = ctx->stream;
    PTSwap sw;
    sw.E = P->d_E;
    sw.M = P->d_neq;
    sw.T = P->d_T;
    sw.was = P->d_was;
    sw.slot = P->d_slot;
    sw.flag = P->d_flag;
    sw.att = P->d_att;
    sw.acc = P->d_acc;
    sw.trips = P->d_trips;
    sw.R = R;
    sw.do_swap = do_swap ? 1 : 0;
    sw.k0 = P->key0;
    sw.k1 = P->key1;
    sw.nl = nl;
    sw.skey = nullptr;
    const unsigned tblocks = reduce_blocks(P->sites);
    for (int t = 0; t < n_rounds; ++t) {
        ptp_sweeps(P, swap_interval, small);
        P->sweeps += (uint64_t)swap_interval;
        if (do_swap || record) {
            ptp_enqueue_measure(P);
            const size_t row = (size_t)t * P->nw;
            sw.hE = record ? P->d_hE + row : nullptr;
            sw.hM = record ? P->d_hM + row : nullptr;
            sw.hW = record ? P->d_hW + row : nullptr;
            sw.t = P->rounds;
            pt_enqueue_swap(sw, (unsigned)nl, st);
            P->launches += 1;
            if (record) {
                const int words = P->nw * TSU_POTTS_MAX_Q;
                hipLaunchKernelGGL(k13_pt_gather, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, P->d_N, P->d_was, R, words,
                                   P->d_hN + row * TSU_POTTS_MAX_Q);
                P->launches += 1;
                if (nl == 2) {
                    hipLaunchKernelGGL(k13_pt_table, dim3(tblocks, (unsigned)R), dim3(256), 0, st, P->d_s, P->d_was, R, P->sites, q,
                                       reinterpret_cast<unsigned long long*>(P->d_hC + (size_t)t * R * q * q));
                    P->launches += 1;
                }
            }
        }
        P->rounds += 1;
    }
    TSU_HIP_TRY(ctx, hipGetLastError());
    return TSU_OK;
}

int tsu_potts_pt_history(tsu_potts_pt* P, double* E, int64_t* n_eq, int64_t* N, int32_t* walker) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    const size_t n = (size_t)P->hist_rounds * P->nw;
    if (n) {
        if (E) TSU_HIP_TRY(ctx, hipMemcpyAsync(E, P->d_hE, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (n_eq) TSU_HIP_TRY(ctx, hipMemcpyAsync(n_eq, P->d_hM, n * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        if (N) TSU_HIP_TRY(ctx, hipMemcpyAsync(N, P->d_hN, n * TSU_POTTS_MAX_Q * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        if (walker) TSU_HIP_TRY(ctx, hipMemcpyAsync(walker, P->d_hW, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int tsu_potts_pt_overlap_tables(tsu_potts_pt* P, int64_t* tables) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, P->nl == 2, "potts_pt_overlap_tables: the tables need two ladders");
    TSU_REQUIRE(ctx, tables || P->hist_rounds == 0, "potts_pt_overlap_tables: tables is NULL");
    const size_t n = (size_t)P->hist_rounds * P->R * P->q * P->q;
    if (n) TSU_HIP_TRY(ctx, hipMemcpyAsync(tables, P->d_hC, n * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int tsu_potts_pt_stats(tsu_potts_pt* P, int64_t* attempts, int64_t* accepts, int64_t* round_trips, int32_t* walker_at_slot,
                       uint64_t* sweep_count, uint64_t* round_count) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    const size_t pairs = (size_t)P->nl * (P->R - 1), nw = (size_t)P->nw;
    if (attempts) TSU_HIP_TRY(ctx, hipMemcpyAsync(attempts, P->d_att, pairs * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (accepts) TSU_HIP_TRY(ctx, hipMemcpyAsync(accepts, P->d_acc, pairs * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (round_trips) TSU_HIP_TRY(ctx, hipMemcpyAsync(round_trips, P->d_trips, nw * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (walker_at_slot) TSU_HIP_TRY(ctx, hipMemcpyAsync(walker_at_slot, P->d_was, nw * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (sweep_count) *sweep_count = P->sweeps;
    if (round_count) *round_count = P->rounds;
    return TSU_OK;
}

int tsu_potts_pt_energies(tsu_potts_pt* P, double* E, int64_t* n_eq) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, P->have_disorder, "potts_pt_energies: call tsu_potts_pt_set_disorder first");
    ptp_enqueue_measure(P);
    TSU_HIP_TRY(ctx, hipGetLastError());
    const size_t nw = (size_t)P->nw;
    if (E) TSU_HIP_TRY(ctx, hipMemcpyAsync(E, P->d_E, nw * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (n_eq) TSU_HIP_TRY(ctx, hipMemcpyAsync(n_eq, P->d_neq, nw * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int tsu_potts_pt_route(tsu_potts_pt* P, int* route) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P || !route) return TSU_E_INVALID;
    *route = ptp_small_route(P) ? TSU_POTTS_PT_ROUTE_SMALL : TSU_POTTS_PT_ROUTE_SWEEP;
    return TSU_OK;
}

int tsu_potts_pt_launch_count(tsu_potts_pt* P, uint64_t* n) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P || !n) return TSU_E_INVALID;
    *n = P->launches;
    return TSU_OK;
}

}  // extern "C"

// pte_host.h -- the host side of a tempering ensemble (tsu_pte2d, ising2d_disorder.hip; tsu_pte3d, ising3d.hip): S disorder samples
// x nl ladders x R temperatures of one lattice shape in one handle ("Tempering ensembles").  The handle is
// pt_ladder.h's ladder with S samples, so the run loop, history, stats, energies and the recording switches are pt_host.h's as they
// stand; what differs from a ladder handle is here: the storage (as pop_host.h: all spin planes in one allocation, no lattice handle
// per walker, and all disorder in one allocation), the per-sample seeds, and the start of all walkers in one launch.  A handle type
// derives from pte_handle and adds `lat`, one lattice handle that gives the shape its validation and a sample's disorder its checks.
// Messages carry the handle's name ("pte2d" / "pte3d").  Internal linkage throughout.
//
// Memory: S nl R planes of nrows pitch bytes; S n_dis planes of fp32 disorder; the energy partials keep the kernels' fixed stride of
// kEnergyBlocks per walker: 8 KiB of float64 partials and 8 KiB of int64 ones, 128 MiB + 128 MiB at 16 384 walkers and
// 512 MiB + 512 MiB at the limit of 65 535.
#pragma once
#include <new>
#include <vector>

#include "disorder_dev.h"
#include "pt_host.h"

constexpr int kPteMaxWalkers = 65535;  // grid y of the energy partial pass

struct pte_handle : pt_ladder {
    size_t plane;       // nrows * pitch: elements of a spin plane and of a disorder plane
    int8_t* d_pool;     // [walker][plane]
    float* d_dis;       // [sample][J_right, J_down, (J_layer,) h][plane], the lattice's layout per sample
    int n_dis;          // disorder planes per sample: 3 (2-D) or 4 (3-D)
    int have_disorder;
};

namespace {

// the handle with its planes, disorder, tables and history, and its lattice (destroy(lat) frees it)
template <class H, class Destroy>
void pte_delete(H* P, Destroy destroy) {
    if (P->d_pool) (void)hipFree(P->d_pool);
    if (P->d_dis) (void)hipFree(P->d_dis);
    pt_free_tables(P);
    if (P->lat) (void)destroy(P->lat);
    delete P;
}

// create: the limits (before anything is allocated), the handle H (a pte_handle with the lattice `lat`), make(P) creates the lattice
// (its own shape checks and messages) and fills the shape and n_dis, then the planes, the disorder and the tables.  An ensemble
// that does not fit leaves nothing behind (free_handle(P)), HIP's last error included.
template <class H, class Make, class Free>
int pte_create(tsu_ctx* ctx, const char* name, int n_samples, int n_temps, int n_ladders, H** out, Make make, Free free_handle) {
    *out = nullptr;
    TSU_REQUIRE(ctx, n_samples >= 1, "%s_create: n_samples must be >= 1, got %d", name, n_samples);
    TSU_REQUIRE(ctx, n_temps >= 2 && n_temps <= kPtMaxTemps, "%s_create: n_temps must be in [2, %d], got %d", name, kPtMaxTemps, n_temps);
    TSU_REQUIRE(ctx, n_ladders == 1 || n_ladders == 2, "%s_create: n_ladders must be 1 or 2, got %d", name, n_ladders);
    // the sweep's grid z is S ceil(nl R / W) <= S nl R groups: the same bound covers it for every W
    TSU_REQUIRE(ctx, (long long)n_samples * n_ladders * n_temps <= kPteMaxWalkers,
                "%s_create: %d samples x %d ladder(s) x %d temperatures = %lld walkers, more than the %d one launch covers", name, n_samples,
                n_ladders, n_temps, (long long)n_samples * n_ladders * n_temps, kPteMaxWalkers);
    H* P = new (std::nothrow) H();
    if (!P) return tsu_fail(ctx, TSU_E_NOMEM, "%s_create: host allocation failed", name);
    P->ctx = ctx;
    P->name = name;
    P->R = n_temps;
    P->nl = n_ladders;
    P->S = n_samples;
    P->nw = n_samples * n_ladders * n_temps;
    int rc = make(P);
    if (rc == TSU_OK) {
        const size_t nw = (size_t)P->nw;
        P->plane = (size_t)P->nrows * (size_t)P->pitch;
        const size_t dis = (size_t)P->S * P->n_dis * P->plane * sizeof(float);
        hipError_t e = hipMalloc((void**)&P->d_pool, nw * P->plane);
        if (e == hipSuccess) e = hipMalloc((void**)&P->d_dis, dis);
        if (e == hipSuccess) e = hipMalloc((void**)&P->d_skey, 2 * (size_t)P->S * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemsetAsync(P->d_pool, 0, nw * P->plane, ctx->stream);  // pad bytes stay 0
        if (e == hipSuccess) e = hipMemsetAsync(P->d_dis, 0, dis, ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(P->d_skey, 0, 2 * (size_t)P->S * sizeof(uint32_t), ctx->stream);
        if (e != hipSuccess) {
            rc = tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "%s_create: %d planes of %zu bytes, %zu bytes of disorder: %s",
                          name, P->nw, P->plane, dis, hipGetErrorString(e));
            (void)hipStreamSynchronize(ctx->stream);
        } else {
            std::vector<int8_t*> planes(nw);
            for (size_t g = 0; g < nw; ++g) planes[g] = P->d_pool + g * P->plane;
            rc = pt_alloc_tables(P, planes.data());  // synchronises
        }
    }
    if (rc != TSU_OK) {
        free_handle(P);
        (void)hipGetLastError();
        return rc;
    }
    *out = P;
    return TSU_OK;
}

// set_disorder: src[j] = [S][shape] arrays in the lattice's order, the field last and nullable.  set(lat, ptrs) is the lattice's own
// set_disorder (checks, messages, its device layout with the pads 0) and lat_dis_of(P) where it stores them; each sample passes
// through it and is copied on the device into its place.  An error leaves the handle without disorder (synchronises).
template <class H, class Dis, class Set>
int pte_set_disorder(H* P, const float* const* src, size_t sites, Dis lat_dis_of, Set set) {
    tsu_ctx* ctx = P->ctx;
    const int n = P->n_dis;
    for (int j = 0; j + 1 < n; ++j) TSU_REQUIRE(ctx, src[j], "%s_set_disorder: the coupling arrays are required (h may be NULL)", P->name);
    P->have_disorder = 0;
    const size_t per = (size_t)n * P->plane;
    for (int s = 0; s < P->S; ++s) {
        const float* one[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int j = 0; j < n; ++j) one[j] = src[j] ? src[j] + (size_t)s * sites : nullptr;
        const int rc = set(P->lat, one);  // synchronises
        if (rc != TSU_OK) return rc;
        TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_dis + (size_t)s * per, lat_dis_of(P), per * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // before the next sample overwrites the lattice's copy
    }
    P->have_disorder = 1;
    return TSU_OK;
}

// init: walker (s, k, w) gets the key seeds[s] + k R + w and the lattice's start with it (random: one launch for all walkers; up /
// down: one fill launch), sample s the swap key seeds[s]; tables and counters reset (synchronises)
int pte_init(pte_handle* P, const uint64_t* seeds, int initial) {
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, seeds, "%s_init: NULL seeds", P->name);
    TSU_REQUIRE(ctx, initial == 0 || initial == 1 || initial == -1, "%s_init: initial must be 0 (random), 1 (up) or -1 (down), got %d",
                P->name, initial);
    P->have_init = 0;
    const int per = P->nl * P->R;
    std::vector<uint32_t> key(2 * (size_t)P->nw), skey(2 * (size_t)P->S);
    for (int s = 0; s < P->S; ++s) {
        skey[2 * s] = (uint32_t)seeds[s];
        skey[2 * s + 1] = (uint32_t)(seeds[s] >> 32);
        for (int i = 0; i < per; ++i) {
            const uint64_t k = seeds[s] + (uint64_t)i;
            const size_t g = (size_t)s * per + i;
            key[2 * g] = (uint32_t)k;
            key[2 * g + 1] = (uint32_t)(k >> 32);
        }
    }
    TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_key, key.data(), key.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_skey, skey.data(), skey.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    const dim3 grid((unsigned)((pt_lanes(P) + 255) / 256), (unsigned)P->nw, 1);
    if (initial == 0) pt_randomize_all<<<grid, 256, 0, ctx->stream>>>(P->d_s, P->d_key, P->nrows, P->pitch, P->cols);
    else pt_fill_all<<<grid, 256, 0, ctx->stream>>>(P->d_s, initial, P->nrows, P->pitch, P->cols);
    TSU_HIP_TRY(ctx, hipGetLastError());
    const int rc = pt_reset(P);  // synchronises before the keys go
    if (rc != TSU_OK) return rc;
    P->key0 = skey[0];
    P->key1 = skey[1];
    P->have_init = 1;
    return TSU_OK;
}

// g = the walker now at (sample, ladder, slot), an index into the planes; `op` names the entry point (synchronises)
int pte_at(pte_handle* P, int sample, int ladder, int slot, const char* op, size_t* g) {
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, sample >= 0 && sample < P->S && ladder >= 0 && ladder < P->nl && slot >= 0 && slot < P->R,
                "%s_%s: sample %d, ladder %d, slot %d out of range (%d sample(s) of %d ladder(s) of %d temperatures)", P->name, op, sample,
                ladder, slot, P->S, P->nl, P->R);
    const size_t row = ((size_t)sample * P->nl + ladder) * P->R;
    int32_t w = -1;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(&w, P->d_was + row + slot, sizeof(w), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (w < 0 || w >= P->R) return tsu_fail(ctx, TSU_E_HIP, "%s_%s: corrupt slot table (walker %d)", P->name, op, (int)w);
    *g = row + (size_t)w;
    return TSU_OK;
}

int pte_get_spins(pte_handle* P, int sample, int ladder, int slot, int8_t* host) {
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, host, "%s_get_spins: NULL output", P->name);
    size_t g = 0;
    const int rc = pte_at(P, sample, ladder, slot, "get_spins", &g);
    if (rc != TSU_OK) return rc;
    TSU_HIP_TRY(ctx, hipMemcpy2DAsync(host, (size_t)P->cols, P->d_pool + g * P->plane, (size_t)P->pitch, (size_t)P->cols, (size_t)P->nrows,
                                      hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int pte_set_spins(pte_handle* P, int sample, int ladder, int slot, const int8_t* host) {
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, host, "%s_set_spins: NULL input", P->name);
    size_t g = 0;
    const int rc = pte_at(P, sample, ladder, slot, "set_spins", &g);
    if (rc != TSU_OK) return rc;
    TSU_HIP_TRY(ctx, hipMemcpy2DAsync(P->d_pool + g * P->plane, (size_t)P->pitch, host, (size_t)P->cols, (size_t)P->cols, (size_t)P->nrows,
                                      hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

// what the ensemble kernels take beside the ladders' parameters (disorder_dev.h) at W walkers per lane: the sweep's grid z is groups
// of W walkers within each sample's nl R walkers, a sample's disorder its n_dis planes
PTEns pte_ens(const pte_handle* P, int W) {
    PTEns e;
    e.dstride = (long long)P->n_dis * (long long)P->plane;
    e.nper = P->nl * P->R;
    e.groups = (e.nper + W - 1) / W;
    return e;
}

}  // namespace

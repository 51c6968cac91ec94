// pt_host.h -- the host side of a parallel-tempering handle, once for the 2-D ladders (tsu_pt2d, ising2d_pt.h / ising2d_disorder.hip)
// and the 3-D ladders (tsu_pt3d, ising3d.hip): free functions on pt_ladder (pt_ladder.h), which holds what both handles have.  A
// handle type derives from it (plain struct inheritance) and adds its walkers `lat` and whatever only its dimension has.  The
// dimension passes in how it launches a half-sweep and an energy partial pass, and a hook a round runs between the two;
// everything else of create, set_temperatures, init, run, history, stats and energies is here.  Messages carry the ladder's name
// ("pt2d" / "pt3d") as their prefix.  Internal linkage throughout, as pt_dev.h.
//
// A pt_ladder holds S disorder samples (pt_ladder.h): 1 for the two ladder handles, any number for a tempering ensemble (pte_host.h,
// "pte2d" / "pte3d"), which brings its own create, set_disorder and init and shares everything else here.  Every table, history row
// and launch below is sized by S, with the sample as the leading index; with S = 1 they are what they were.
#pragma once
#include <cmath>
#include <cstdlib>
#include <new>
#include <type_traits>
#include <vector>

#include "corr_dev.h"
#include "link_dev.h"
#include "pt_ladder.h"
#include "reduce_dev.h"

namespace {

void pt_free_history(pt_ladder* P) {
    void* bufs[] = {P->d_hE, P->d_hM, P->d_hW, P->d_hq, P->d_hF, P->d_hL};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    P->d_hE = nullptr;
    P->d_hM = nullptr;
    P->d_hW = nullptr;
    P->d_hq = nullptr;
    P->d_hF = nullptr;
    P->d_hL = nullptr;
    P->hist_cap = 0;
}

// the tables and the history
void pt_free_tables(pt_ladder* P) {
    void* bufs[] = {P->d_s, P->d_key, P->d_slot, P->d_was, P->d_flag, P->d_T, P->d_c32, P->d_att, P->d_acc,
                    P->d_trips, P->d_part, P->d_ipart, P->d_E, P->d_M, P->d_prof, P->d_tab, P->d_skey};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    pt_free_history(P);
}

// the handle with its tables, history and walkers (destroy(lat[g]) frees one)
template <class H, class Destroy>
void pt_delete(H* P, Destroy destroy) {
    pt_free_tables(P);
    if (P->lat) {
        for (int g = 0; g < P->nw; ++g)
            if (P->lat[g]) (void)destroy(P->lat[g]);
        delete[] P->lat;
    }
    delete P;
}

// every walker at its own slot, the walker at slot 0 "bottom", no attempts, accepts or round trips (synchronises)
int pt_reset(pt_ladder* P) {
    tsu_ctx* ctx = P->ctx;
    const int R = P->R, nl = P->S * P->nl;  // the ladders of all samples
    std::vector<int32_t> ident((size_t)nl * R), flag((size_t)nl * R, kPtNone);
    for (int k = 0; k < nl; ++k) {
        for (int w = 0; w < R; ++w) ident[(size_t)k * R + w] = w;
        flag[(size_t)k * R] = kPtBottom;
    }
    const size_t b = (size_t)nl * R * sizeof(int32_t);
    TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_slot, ident.data(), b, hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_was, ident.data(), b, hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_flag, flag.data(), b, hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_att, 0, (size_t)nl * (R - 1) * sizeof(long long), ctx->stream));
    TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_acc, 0, (size_t)nl * (R - 1) * sizeof(long long), ctx->stream));
    TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_trips, 0, (size_t)nl * R * sizeof(long long), ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    P->sweeps = P->rounds = 0;
    P->hist_rounds = 0;
    return TSU_OK;
}

// the device tables of a ladder whose walkers exist (planes[g] = walker g's spin plane), reset (synchronises)
int pt_alloc_tables(pt_ladder* P, int8_t* const* planes) {
    tsu_ctx* ctx = P->ctx;
    const size_t nw = (size_t)P->nw, nlR = nw, R = (size_t)P->R;
    hipError_t e = hipSuccess;
    auto alloc = [&e](auto*& ptr, size_t bytes) {
        if (e == hipSuccess) e = hipMalloc((void**)&ptr, bytes);
    };
    alloc(P->d_s, nw * sizeof(int8_t*));
    alloc(P->d_key, 2 * nw * sizeof(uint32_t));
    alloc(P->d_slot, nlR * sizeof(int32_t));
    alloc(P->d_was, nlR * sizeof(int32_t));
    alloc(P->d_flag, nlR * sizeof(int32_t));
    alloc(P->d_T, R * sizeof(double));
    alloc(P->d_c32, R * sizeof(float));
    alloc(P->d_att, (size_t)P->S * P->nl * (R - 1) * sizeof(long long));
    alloc(P->d_acc, (size_t)P->S * P->nl * (R - 1) * sizeof(long long));
    alloc(P->d_trips, nlR * sizeof(long long));
    alloc(P->d_part, nw * kEnergyBlocks * sizeof(double));
    alloc(P->d_ipart, nw * kEnergyBlocks * sizeof(long long));
    alloc(P->d_E, nw * sizeof(double));
    alloc(P->d_M, nw * sizeof(long long));
    if (e == hipSuccess) e = hipMemcpyAsync(P->d_s, planes, nw * sizeof(int8_t*), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(P->d_key, 0, 2 * nw * sizeof(uint32_t), ctx->stream);
    if (e != hipSuccess) {
        const int rc = tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "%s_create: %s", P->name, hipGetErrorString(e));
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    return pt_reset(P);  // synchronises before the caller's `planes` goes
}

// create: the checks, the handle H (a pt_ladder with walkers `lat`), its walkers (make(&lat[g]) creates one, with the lattice's own
// shape checks and messages), then shape(P, planes), which fills nrows / pitch / cols and the walkers' spin planes, and the tables.
// A ladder that does not fit leaves nothing behind (free_handle(P)), HIP's last error included.
template <class H, class Make, class Shape, class Free>
int pt_create(tsu_ctx* ctx, const char* name, int n_temps, int n_ladders, H** out, Make make, Shape shape, Free free_handle) {
    *out = nullptr;
    TSU_REQUIRE(ctx, n_temps >= 2 && n_temps <= kPtMaxTemps, "%s_create: n_temps must be in [2, %d], got %d", name, kPtMaxTemps, n_temps);
    TSU_REQUIRE(ctx, n_ladders == 1 || n_ladders == 2, "%s_create: n_ladders must be 1 or 2, got %d", name, n_ladders);
    H* P = new (std::nothrow) H();
    if (!P) return tsu_fail(ctx, TSU_E_NOMEM, "%s_create: host allocation failed", name);
    P->ctx = ctx;
    P->name = name;
    P->R = n_temps;
    P->nl = n_ladders;
    P->S = 1;
    P->nw = n_temps * n_ladders;
    P->lat = new (std::nothrow) std::remove_pointer_t<decltype(P->lat)>[P->nw]();
    int rc = P->lat ? TSU_OK : tsu_fail(ctx, TSU_E_NOMEM, "%s_create: host allocation failed", name);
    for (int g = 0; rc == TSU_OK && g < P->nw; ++g) rc = make(&P->lat[g]);
    if (rc == TSU_OK) {
        std::vector<int8_t*> planes((size_t)P->nw);
        shape(P, planes.data());
        rc = pt_alloc_tables(P, planes.data());
    }
    if (rc != TSU_OK) {
        free_handle(P);
        (void)hipGetLastError();
        return rc;
    }
    *out = P;
    return TSU_OK;
}

// lanes of a pass over one walker: a lane per chunk of 16 columns
long long pt_lanes(const pt_ladder* P) { return P->nrows * ((P->cols + 15) / 16); }

// Walkers per lane of the ladder sweeps (k7_pt_sweep, k8_pt_sweep): the fewest groups that still give >= 1024 lanes per CU (a
// lane per octet and group), so a large lattice reads each octet's disorder once for many walkers and a small one spreads its
// walkers over the chip.  TSU_PT_GROUP=w (read per call) forces w.  An ensemble counts the walkers of all its samples here and
// keeps a group within one sample's walkers (pt_group).
int pt_group_of(const tsu_ctx* ctx, long long lanes, int nw) {
    if (const char* e = getenv("TSU_PT_GROUP")) {
        const int w = atoi(e);
        if (w >= 1) return w < nw ? w : nw;
    }
    const long long want = (long long)(ctx->cus > 0 ? ctx->cus : 256) * 1024;
    const long long groups = (want + lanes - 1) / lanes;
    if (groups >= nw) return 1;
    return (int)((nw + groups - 1) / groups);
}

int pt_group(const pt_ladder* P) {
    const int w = pt_group_of(P->ctx, pt_lanes(P), P->nw), per = P->nl * P->R;
    return w < per ? w : per;
}

int pt_set_temperatures(pt_ladder* P, const double* T) {
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, T, "%s_set_temperatures: NULL temperatures", P->name);
    double t[kPtMaxTemps];
    float c[kPtMaxTemps];
    for (int i = 0; i < P->R; ++i) {
        TSU_REQUIRE(ctx, T[i] > 0.0 && std::isfinite(T[i]), "Temperature must be positive (%s_set_temperatures: T[%d] = %g)", P->name, i,
                    T[i]);
        t[i] = T[i];
        c[i] = (float)(2.0 / T[i]);
    }
    for (int i = 0; i < P->R; ++i) P->h_T[i] = t[i];
    TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_T, t, P->R * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_c32, c, P->R * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    P->have_T = 1;
    return TSU_OK;
}

// init: walker g starts from start(g, seed + g) (the single-lattice scan's model g) with the Philox key seed + g; tables reset, then
// after() (what else the dimension resets; returns a status).  The handle counts as initialised only once all of it succeeded.
template <class Start, class After>
int pt_init(pt_ladder* P, uint64_t seed, int initial, Start start, After after) {
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, initial == 0 || initial == 1 || initial == -1, "%s_init: initial must be 0 (random), 1 (up) or -1 (down), got %d",
                P->name, initial);
    std::vector<uint32_t> key(2 * (size_t)P->nw);
    for (int g = 0; g < P->nw; ++g) {
        const uint64_t s = seed + (uint64_t)g;
        key[2 * g] = (uint32_t)s;
        key[2 * g + 1] = (uint32_t)(s >> 32);
        const int rc = start(g, s);
        if (rc != TSU_OK) return rc;
    }
    TSU_HIP_TRY(ctx, hipMemcpyAsync(P->d_key, key.data(), key.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    int rc = pt_reset(P);  // synchronises before `key` goes
    if (rc != TSU_OK) return rc;
    rc = after();
    if (rc != TSU_OK) return rc;
    P->key0 = (uint32_t)seed;
    P->key1 = (uint32_t)(seed >> 32);
    P->have_init = 1;
    return TSU_OK;
}

// every walker's E and sum of spins into d_E / d_M (asynchronous); partials(blocks) enqueues the dimension's partial pass of
// `blocks` workgroups per walker into d_part / d_ipart
template <class Partials>
void pt_enqueue_energies(pt_ladder* P, unsigned blocks, Partials&& partials) {
    partials(blocks);
    pt_energy_final<<<(unsigned)P->nw, 256, 0, P->ctx->stream>>>(P->d_part, P->d_ipart, (int)blocks, P->d_E, P->d_M);
}

// the swap pass of `rows` ladders (one workgroup each) on `st`: the one launch of k7_pt_swap, for the lattice handles' rounds below and
// for the walker batches on a sparse graph (sparse_batch.hip), which fill a PTSwap from tables of their own
inline void pt_enqueue_swap(const PTSwap& sw, unsigned rows, hipStream_t st) { k7_pt_swap<<<rows, 64, 0, st>>>(sw); }

// ---------------------------------------------------------------- correlation recording (corr_dev.h)
// (templates: the population handle, pop_host.h, keeps its axes under the same names)
template <class H>
long long pt_prof_len(const H* P) {
    long long n = 0;
    for (int a = 0; a < P->n_axes; ++a) n += P->axis_len[a];
    return n;
}

template <class H>
int pt_periodic_axes(const H* P) {
    int n = 0;
    for (int a = 0; a < P->n_axes; ++a) n += P->axis_per[a] ? 1 : 0;
    return n;
}

// doubles of a slot's modes: (re, im) per periodic axis
template <class H>
size_t pt_mode_doubles(const H* P) { return 2 * (size_t)pt_periodic_axes(P); }

dim3 pt_profile_plan(const pt_ladder* P, ProfArgs& pa) {
    return profile_plan(pa, P->pitch, P->pitch, P->nrows, P->lrows, P->cols, P->n_axes == 3, (unsigned)(P->S * P->R));
}

// where the mode pass finds each periodic axis's profile and tables
template <class H>
ModeArgs pt_mode_args(const H* P) {
    ModeArgs m = {};
    int off = 0;
    const double* tab = P->d_tab;
    for (int a = 0; a < P->n_axes; ++a) {
        if (P->axis_per[a]) {
            m.off[m.n] = off;
            m.len[m.n] = P->axis_len[a];
            m.cs[m.n] = tab;
            m.sn[m.n] = tab + P->axis_len[a];
            tab += 2 * (size_t)P->axis_len[a];
            m.n += 1;
        }
        off += P->axis_len[a];
    }
    return m;
}

int pt_prof_scratch(pt_ladder* P, const char* op) {
    if (P->d_prof) return TSU_OK;
    const hipError_t e = hipMalloc((void**)&P->d_prof, (size_t)P->S * P->R * pt_prof_len(P) * sizeof(long long));
    if (e == hipSuccess) return TSU_OK;
    (void)hipGetLastError();
    return tsu_fail(P->ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "%s_%s: %s", P->name, op, hipGetErrorString(e));
}

// set_correlation: cs[a] / sn[a] = the host's cos / sin tables of axis a (both NULL exactly on an open axis).  Switching it on drops
// the recorded history (its buffers gain the modes with the next run); switching it off leaves a run what it was (synchronises)
int pt_set_correlation(pt_ladder* P, int enable, const double* const* cs, const double* const* sn) {
    tsu_ctx* ctx = P->ctx;
    if (!enable) {
        P->corr = 0;
        return TSU_OK;
    }
    TSU_REQUIRE(ctx, pt_periodic_axes(P) > 0, "%s_set_correlation: the lattice has no periodic axis (no k_min mode is defined)", P->name);
    size_t n = 0;
    for (int a = 0; a < P->n_axes; ++a) {
        if (P->axis_per[a]) {
            TSU_REQUIRE(ctx, cs[a] && sn[a], "%s_set_correlation: NULL table of periodic axis %d", P->name, a);
            n += 2 * (size_t)P->axis_len[a];
        } else {
            TSU_REQUIRE(ctx, !cs[a] && !sn[a], "%s_set_correlation: axis %d is open: its tables must be NULL", P->name, a);
        }
    }
    int rc = pt_prof_scratch(P, "set_correlation");
    if (rc != TSU_OK) return rc;
    if (!P->d_tab) {
        const hipError_t e = hipMalloc((void**)&P->d_tab, n * sizeof(double));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "%s_set_correlation: %s", P->name, hipGetErrorString(e));
        }
    }
    double* tab = P->d_tab;
    for (int a = 0; a < P->n_axes; ++a)
        if (P->axis_per[a]) {
            const size_t len = (size_t)P->axis_len[a];
            TSU_HIP_TRY(ctx, hipMemcpyAsync(tab, cs[a], len * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            TSU_HIP_TRY(ctx, hipMemcpyAsync(tab + len, sn[a], len * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            tab += 2 * len;
        }
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // before the caller's tables go
    if (!P->corr) {
        pt_free_history(P);
        P->hist_rounds = 0;
        P->hist_modes = 0;
    }
    P->corr = 1;
    return TSU_OK;
}

// the modes of the last run's rows, [round][sample][slot][periodic axis][re, im] (synchronises)
int pt_history_modes(pt_ladder* P, double* modes) {
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, modes, "%s_history_modes: NULL output", P->name);
    TSU_REQUIRE(ctx, P->hist_modes, "%s_history_modes: the last run recorded no modes (call tsu_%s_set_correlation before a recording run)",
                P->name, P->name);
    const size_t n = (size_t)P->hist_rounds * P->S * P->R * pt_mode_doubles(P);
    if (n) TSU_HIP_TRY(ctx, hipMemcpyAsync(modes, P->d_hF, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

// the profiles of the walkers of `sample` now at `slot` (the product of the two ladders' walkers if there are two), axis a into
// out[a] (synchronises)
int pt_profiles(pt_ladder* P, int slot, int64_t* const* out, int sample = 0) {
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, sample >= 0 && sample < P->S, "%s_profiles: sample %d out of range (%d samples)", P->name, sample, P->S);
    TSU_REQUIRE(ctx, slot >= 0 && slot < P->R, "%s_profiles: slot %d out of range (%d temperatures)", P->name, slot, P->R);
    for (int a = 0; a < P->n_axes; ++a) TSU_REQUIRE(ctx, out[a], "%s_profiles: NULL output", P->name);
    const int rc = pt_prof_scratch(P, "profiles");
    if (rc != TSU_OK) return rc;
    const long long len = pt_prof_len(P);
    ProfArgs pa;
    const dim3 grid = pt_profile_plan(P, pa);
    TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_prof, 0, (size_t)P->S * P->R * len * sizeof(long long), ctx->stream));
    pt_profile<<<grid, 256, 0, ctx->stream>>>(P->d_s, P->d_was, P->R, P->nl, pa, P->d_prof, len);
    TSU_HIP_TRY(ctx, hipGetLastError());
    const long long* row = P->d_prof + ((size_t)sample * P->R + slot) * len;
    for (int a = 0; a < P->n_axes; ++a) {
        TSU_HIP_TRY(ctx, hipMemcpyAsync(out[a], row, (size_t)P->axis_len[a] * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        row += P->axis_len[a];
    }
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

// ---------------------------------------------------------------- link-overlap recording (link_dev.h)
// the launch shape of a link pass over the handle's planes (H: a ladder or a population)
template <class H>
unsigned pt_link_plan(const H* P, LinkArgs& la) {
    const int three = P->n_axes == 3;
    return link_plan(la, P->pitch, P->pitch, P->nrows, P->lrows, P->cols, three ? P->axis_per[0] : 0, P->axis_per[three ? 1 : 0],
                     P->axis_per[three ? 2 : 1]);
}

// set_link_overlap: switching it on drops the recorded history (its buffers gain the L rows with the next run)
int pt_set_link_overlap(pt_ladder* P, int enable) {
    tsu_ctx* ctx = P->ctx;
    if (!enable) {
        P->link = 0;
        return TSU_OK;
    }
    TSU_REQUIRE(ctx, P->nl == 2, "%s_set_link_overlap: the link overlap needs two ladders (this handle has %d)", P->name, P->nl);
    if (!P->link) {
        TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // no kernel still writes the rows
        pt_free_history(P);
        P->hist_rounds = 0;
        P->hist_modes = 0;
        P->hist_link = 0;
    }
    P->link = 1;
    return TSU_OK;
}

// L of the last run's rows, [round][sample][slot] (synchronises)
int pt_history_link(pt_ladder* P, int64_t* L) {
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, L, "%s_history_link: NULL output", P->name);
    TSU_REQUIRE(ctx, P->hist_link, "%s_history_link: the last run recorded no link overlap (call tsu_%s_set_link_overlap before a recording run)",
                P->name, P->name);
    const size_t n = (size_t)P->hist_rounds * P->S * P->R;
    if (n) TSU_HIP_TRY(ctx, hipMemcpyAsync(L, P->d_hL, n * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

// what a run needs, in the order the messages are promised
int pt_run_check(pt_ladder* P, int have_disorder, int n_rounds, int swap_interval) {
    tsu_ctx* ctx = P->ctx;
    const char* nm = P->name;
    TSU_REQUIRE(ctx, have_disorder, "%s_run: call tsu_%s_set_disorder first", nm, nm);
    TSU_REQUIRE(ctx, P->have_T, "%s_run: call tsu_%s_set_temperatures first", nm, nm);
    TSU_REQUIRE(ctx, P->have_init, "%s_run: call tsu_%s_init first", nm, nm);
    TSU_REQUIRE(ctx, n_rounds >= 0 && swap_interval >= 1, "%s_run: need n_rounds >= 0 and swap_interval >= 1 (got %d, %d)", nm, n_rounds,
                swap_interval);
    TSU_REQUIRE(ctx, (uint64_t)P->sweeps + (uint64_t)n_rounds * (uint64_t)swap_interval <= (1ull << 31), "%s_run: sweep counter overflow", nm);
    TSU_REQUIRE(ctx, (uint64_t)P->rounds + (uint64_t)n_rounds <= 0xFFFFFFFFull, "%s_run: round counter overflow", nm);
    return TSU_OK;
}

// n_rounds rounds after pt_run_check: swap_interval sweeps (sweep(hs, colour) enqueues half-sweep hs of all walkers), hook() (what
// the dimension ends a round's sweeps with; returns a status), then, if the round swaps or records, the energies (partials as for
// pt_enqueue_energies), the swap pass and q.  Every pass covers the S samples of the handle in its one launch: the sample is part
// of a grid index and of the rows (history rows [round][sample][..]).  Nothing here waits for the device.
template <class Sweep, class Partials, class Hook>
int pt_run(pt_ladder* P, int n_rounds, int swap_interval, int do_swap, int record, Sweep&& sweep, Partials&& partials, Hook&& hook) {
    tsu_ctx* ctx = P->ctx;
    const int R = P->R, nl = P->nl;
    const size_t S = (size_t)P->S, SR = S * R;  // samples; the (sample, slot) rows of q, L and the modes
    if (record && P->hist_cap < (size_t)n_rounds) {
        pt_free_history(P);
        const size_t n = (size_t)n_rounds * SR * nl;
        hipError_t e = hipMalloc((void**)&P->d_hE, n * sizeof(double));
        if (e == hipSuccess) e = hipMalloc((void**)&P->d_hM, n * sizeof(long long));
        if (e == hipSuccess) e = hipMalloc((void**)&P->d_hW, n * sizeof(int32_t));
        if (e == hipSuccess) e = hipMalloc((void**)&P->d_hq, (size_t)n_rounds * SR * sizeof(long long));
        if (e == hipSuccess && P->corr) e = hipMalloc((void**)&P->d_hF, (size_t)n_rounds * SR * pt_mode_doubles(P) * sizeof(double));
        if (e == hipSuccess && P->link) e = hipMalloc((void**)&P->d_hL, (size_t)n_rounds * SR * sizeof(long long));
        if (e != hipSuccess) {  // nothing of a history that does not fit stays behind
            pt_free_history(P);
            P->hist_rounds = 0;
            (void)hipGetLastError();
            return tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "%s_run: history of %d rounds: %s", P->name, n_rounds,
                            hipGetErrorString(e));
        }
        P->hist_cap = (size_t)n_rounds;
    }
    // pt_overlap adds into its row: every q row of this run starts at 0
    if (record && nl == 2 && n_rounds > 0)
        TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_hq, 0, (size_t)n_rounds * SR * sizeof(long long), ctx->stream));
    P->hist_rounds = record ? n_rounds : 0;
    P->hist_modes = record && P->corr;
    P->hist_link = record && P->link && nl == 2;
    if (P->hist_link && n_rounds > 0) TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_hL, 0, (size_t)n_rounds * SR * sizeof(long long), ctx->stream));
    LinkArgs la;
    const unsigned lblocks = pt_link_plan(P, la);
    const unsigned blocks = reduce_blocks(pt_lanes(P));
    ProfArgs pa;
    ModeArgs ma = {};
    const dim3 pgrid = pt_profile_plan(P, pa);
    if (P->hist_modes) ma = pt_mode_args(P);
    PTSwap sw;
    sw.E = P->d_E;
    sw.M = P->d_M;
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
    sw.skey = P->d_skey;
    for (int t = 0; t < n_rounds; ++t) {
        for (int s = 0; s < swap_interval; ++s)
            for (int colour = 0; colour < 2; ++colour) {
                sweep(2u * (P->sweeps + (uint32_t)s) + (uint32_t)colour, colour);
                P->launches += 1;
            }
        P->sweeps += (uint32_t)swap_interval;
        const int rc = hook();  // the energies see what it moved
        if (rc != TSU_OK) return rc;
        if (do_swap || record) {
            pt_enqueue_energies(P, blocks, partials);
            const size_t row = (size_t)t * SR * nl;
            sw.hE = record ? P->d_hE + row : nullptr;
            sw.hM = record ? P->d_hM + row : nullptr;
            sw.hW = record ? P->d_hW + row : nullptr;
            sw.t = P->rounds;
            pt_enqueue_swap(sw, (unsigned)(S * nl), ctx->stream);
            if (record && nl == 2)
                pt_overlap<<<dim3(blocks, (unsigned)SR, 1), 256, 0, ctx->stream>>>(P->d_s, P->d_was, R, P->pitch, P->nrows, P->cols,
                                                                                  P->d_hq + (size_t)t * SR);
            if (P->hist_link) pt_link<<<dim3(lblocks, (unsigned)SR, 1), 256, 0, ctx->stream>>>(P->d_s, P->d_was, R, la, P->d_hL + (size_t)t * SR);
            if (P->hist_modes) {  // the walkers the pass left at each slot: their profiles, then the modes of the periodic axes
                TSU_HIP_TRY(ctx, hipMemsetAsync(P->d_prof, 0, SR * pt_prof_len(P) * sizeof(long long), ctx->stream));
                pt_profile<<<pgrid, 256, 0, ctx->stream>>>(P->d_s, P->d_was, R, nl, pa, P->d_prof, pt_prof_len(P));
                pt_modes<<<dim3(2u * (unsigned)ma.n, (unsigned)SR, 1), 256, 0, ctx->stream>>>(
                    P->d_prof, pt_prof_len(P), ma, P->d_hF + (size_t)t * SR * pt_mode_doubles(P));
            }
        }
        P->rounds += 1;
    }
    TSU_HIP_TRY(ctx, hipGetLastError());
    return TSU_OK;
}

int pt_history(pt_ladder* P, double* E, int64_t* M, int64_t* q, int32_t* walker) {
    tsu_ctx* ctx = P->ctx;
    const size_t n = (size_t)P->hist_rounds * P->nw;
    if (n) {
        if (E) TSU_HIP_TRY(ctx, hipMemcpyAsync(E, P->d_hE, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (M) TSU_HIP_TRY(ctx, hipMemcpyAsync(M, P->d_hM, n * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        if (walker) TSU_HIP_TRY(ctx, hipMemcpyAsync(walker, P->d_hW, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        if (q && P->nl == 2)
            TSU_HIP_TRY(ctx, hipMemcpyAsync(q, P->d_hq, (size_t)P->hist_rounds * P->S * P->R * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int pt_stats(pt_ladder* P, int64_t* attempts, int64_t* accepts, int64_t* round_trips, int32_t* walker_at_slot, uint64_t* sweep_count,
             uint64_t* round_count) {
    tsu_ctx* ctx = P->ctx;
    const size_t pairs = (size_t)P->S * P->nl * (P->R - 1), nlR = (size_t)P->nw;
    if (attempts) TSU_HIP_TRY(ctx, hipMemcpyAsync(attempts, P->d_att, pairs * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (accepts) TSU_HIP_TRY(ctx, hipMemcpyAsync(accepts, P->d_acc, pairs * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (round_trips) TSU_HIP_TRY(ctx, hipMemcpyAsync(round_trips, P->d_trips, nlR * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (walker_at_slot)
        TSU_HIP_TRY(ctx, hipMemcpyAsync(walker_at_slot, P->d_was, nlR * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (sweep_count) *sweep_count = P->sweeps;
    if (round_count) *round_count = P->rounds;
    return TSU_OK;
}

// every walker's E and sum of spins now (partials as for pt_enqueue_energies; synchronises)
template <class Partials>
int pt_energies(pt_ladder* P, int have_disorder, double* E, int64_t* sum_s, Partials&& partials) {
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, have_disorder, "%s_energies: call tsu_%s_set_disorder first", P->name, P->name);
    pt_enqueue_energies(P, reduce_blocks(pt_lanes(P)), partials);
    TSU_HIP_TRY(ctx, hipGetLastError());
    if (E) TSU_HIP_TRY(ctx, hipMemcpyAsync(E, P->d_E, (size_t)P->nw * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (sum_s) TSU_HIP_TRY(ctx, hipMemcpyAsync(sum_s, P->d_M, (size_t)P->nw * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

// g = the walker now at (ladder, slot), an index into `lat`; `op` names the entry point ("get_spins") (synchronises)
int pt_at(pt_ladder* P, int ladder, int slot, const char* op, int* g) {
    tsu_ctx* ctx = P->ctx;
    TSU_REQUIRE(ctx, ladder >= 0 && ladder < P->nl && slot >= 0 && slot < P->R,
                "%s_%s: ladder %d, slot %d out of range (%d ladder(s) of %d temperatures)", P->name, op, ladder, slot, P->nl, P->R);
    int32_t w = -1;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(&w, P->d_was + (size_t)ladder * P->R + slot, sizeof(w), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (w < 0 || w >= P->R) return tsu_fail(ctx, TSU_E_HIP, "%s_%s: corrupt slot table (walker %d)", P->name, op, (int)w);
    *g = ladder * P->R + w;
    return TSU_OK;
}

int pt_launch_count(const pt_ladder* P, uint64_t* n) {
    if (!P || !n) return TSU_E_INVALID;
    *n = P->launches;
    return TSU_OK;
}

}  // namespace

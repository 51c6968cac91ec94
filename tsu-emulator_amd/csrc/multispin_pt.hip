// multispin_pt.hip -- K9: parallel tempering of a multispin-coded glass, the swaps on the device (gfx950).
//
// Temperature, threshold table and sweep seed belong to a plane, and the 64 samples of a word swap independently, so a swap
// exchanges configurations, per bit: for two planes x, y of neighbouring slots and a 64-bit accept mask m,
// d = (x ^ y) & m; x ^= d; y ^= d (include/tsu_hip_multispin_pt.h, DESIGN.md section 3 "Tempering of multispin-coded glasses").
//
// A round is: the sweeps (tsu_msc_sweep), one k9_measure into a device row (the record's row, when one is kept), with
// tsu_msc_set_correlation on and a record the k_min modes of the same planes (multispin_corr.hip), k9_pt_plan, k9_pt_apply.
// Nothing comes back to the host inside tsu_msc_pt_run.
//
// k9_pt_plan: one workgroup of four waves per (replica a, word-plane w); lane b of every wave is sample 64 w + b.  The waves copy
// the columns of the row's unsatisfied-bond counts and of the label / flag tables into LDS ([slot][64]).  Wave 0 walks the pairs
// i = 0 .. n_temps - 2 in order, carrying the energy and the label of the configuration that moves up, and decides k7_pt_swap's
// expression in float64; its ballot of the decision (pad lanes never accept) is the pair's mask word M[i][a][w].  The walk is a
// chain of dependent steps of one wave, so everything that does not depend on it is taken off it: the pairs' uniforms,
// dense_uniform(i, round, TSU_TAG_PT_SWAP | a << 8) under the sample's key, are drawn a chunk of 16 pairs ahead by waves 1 .. 3
// into two LDS buffers, and 1 / T[i] - 1 / T[i + 1] comes from the host.  Counters go back to global memory in a coalesced
// pass of all waves after the walk.
//
// k9_pt_apply: one lane per (a, w, site) column, sites fastest.  It streams the column's n_temps words in place,
// cur = x[0]; for i: nxt = x[i + 1]; d = (cur ^ nxt) & M[i]; x[i] = cur ^ d; cur = nxt ^ d; x[last] = cur: one read and one
// write per word, and a configuration climbs as many slots as consecutive pairs accept.  (a, w) is the grid's y, so M[i] is a
// wave-uniform load.
#include <cmath>
#include <new>
#include <vector>

#include "dense.h"  // dense_uniform
#include "multispin_host.h"

struct msc_pt {
    double* d_dbeta;             // pair i -> 1.0 / T[i] - 1.0 / T[i + 1]
    uint32_t* d_skey;            // sample (64 W columns) -> Philox key of its swap uniforms
    uint64_t* d_mask;            // [pair][a][w] accept masks of the current pass
    uint8_t* d_label;            // [a][w][slot][64]: which starting configuration sits at the slot
    uint8_t* d_flag;             // [a][w][label][64]: kNone / kBottom / kTop
    long long* d_trips;          // [a][w][label][64]
    long long* d_att;            // [a][w][pair][64]
    long long* d_acc;
    unsigned long long* d_hist;  // the record of the last run: hist_rows measurement rows (scratch rows after a run without one)
    size_t hist_cap;
    int hist_rows;
    int have_seeds;
    unsigned long long launches;
};

namespace {

constexpr int kScratchRows = 64;     // measurement rows a run without a record cycles through
constexpr int kMscPtMaxTemps = 256;  // labels are bytes; 256 slots x 64 lanes x 8 bytes = 128 KiB of LDS
enum : int { kNone = 0, kBottom = 1, kTop = 2 };

struct MscPtPlan {
    const unsigned long long* row;  // this round's measurement: unsat[(t A + a) W + w][64] first
    const double* dbeta;  // pair i -> 1.0 / T[i] - 1.0 / T[i + 1], divided and subtracted on the host in float64
    const uint32_t* skey;
    uint64_t* mask;
    uint8_t* label;
    uint8_t* flag;
    long long* trips;
    long long* att;
    long long* acc;
    long long nb;
    int nT, A, W, S;
    uint32_t round;
};

constexpr int kPlanWaves = 4;   // wave 0 walks the pairs, the others draw the next chunk's uniforms meanwhile
constexpr int kPlanChunk = 16;  // pairs per chunk: two buffers of 16 x 64 doubles

size_t msc_pt_plan_lds(int nT) { return (size_t)nT * 64 * 8 + (size_t)2 * kPlanChunk * 64 * 8; }

// pt_arrive's rule on a lane's column: a label reaching slot 0 is BOTTOM (a TOP one counts a trip), a BOTTOM label reaching the
// last slot is TOP
__device__ __forceinline__ void msc_pt_arrive(uint8_t* flg, uint8_t* tinc, int label, int slot, int nT, int lane) {
    const int at = label * 64 + lane;
    if (slot == 0) {
        if (flg[at] == kTop) tinc[at] = 1;  // slot 0 is reached through pair 0 only: at most once per pass
        flg[at] = kBottom;
    } else if (slot == nT - 1 && flg[at] == kBottom) {
        flg[at] = kTop;
    }
}

__global__ __launch_bounds__(64 * kPlanWaves) void k9_pt_plan(MscPtPlan p) {
    extern __shared__ __align__(16) unsigned char plan_lds[];
    const int nT = p.nT, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* ubuf = reinterpret_cast<double*>(plan_lds);                            // [2][kPlanChunk][64] uniforms of a chunk of pairs
    uint32_t* e = reinterpret_cast<uint32_t*>(ubuf + 2 * kPlanChunk * 64);         // [slot][64] unsatisfied bonds (at most 3 * 2^30)
    uint8_t* lab = reinterpret_cast<uint8_t*>(e + nT * 64);                        // [slot][64]
    uint8_t* flg = lab + nT * 64;                                                  // [label][64]
    uint8_t* tinc = flg + nT * 64;                                                 // [label][64] trips counted in this pass
    uint8_t* accb = tinc + nT * 64;                                                // [pair][64] accepted in this pass
    const int aw = blockIdx.x, a = aw / p.W, w = aw - a * p.W;
    const int col = 64 * w + lane;
    const bool valid = col < p.S;
    const size_t base = (size_t)aw * nT * 64 + lane;
    for (int t = wave; t < nT; t += kPlanWaves) {
        e[t * 64 + lane] = (uint32_t)p.row[((size_t)(t * p.A + a) * p.W + w) * 64 + lane];
        lab[t * 64 + lane] = p.label[base + (size_t)t * 64];
        flg[t * 64 + lane] = p.flag[base + (size_t)t * 64];
        tinc[t * 64 + lane] = 0;
    }
    const uint32_t k0 = p.skey[2 * col], k1 = p.skey[2 * col + 1];
    const uint32_t tag = TSU_TAG_PT_SWAP | ((uint32_t)a << 8);
    const int npairs = nT - 1, nchunks = (npairs + kPlanChunk - 1) / kPlanChunk;
    // the uniforms of chunk c's pairs first, first + step, ... into buffer c & 1
    auto draw = [&](int c, int first, int step) {
        for (int k = first; k < kPlanChunk; k += step) {
            const int i = c * kPlanChunk + k;
            if (i < npairs) ubuf[((c & 1) * kPlanChunk + k) * 64 + lane] = dense_uniform((uint32_t)i, p.round, tag, k0, k1);
        }
    };
    draw(0, wave, kPlanWaves);
    __syncthreads();
    // the configuration now at slot i: the one that came up from below, if the last pair accepted
    double ex = (double)(2ll * (long long)e[lane] - p.nb);
    int cur = lab[lane];
    for (int c = 0; c < nchunks; ++c) {
        if (wave == 0) {
            const int end = min(npairs, (c + 1) * kPlanChunk);
            for (int i = c * kPlanChunk; i < end; ++i) {
                const double ey = (double)(2ll * (long long)e[(i + 1) * 64 + lane] - p.nb);
                const int nxt = lab[(i + 1) * 64 + lane];
                const double delta = p.dbeta[i] * (ex - ey);
                const double u = ubuf[((c & 1) * kPlanChunk + (i - c * kPlanChunk)) * 64 + lane];
                const bool ok = valid && (delta >= 0.0 || u < exp(delta));
                const unsigned long long m = __ballot(ok);
                if (lane == 0) p.mask[(size_t)i * p.A * p.W + aw] = m;
                accb[i * 64 + lane] = ok ? 1 : 0;
                if (ok) {
                    lab[i * 64 + lane] = (uint8_t)nxt;
                    msc_pt_arrive(flg, tinc, cur, i + 1, nT, lane);
                    msc_pt_arrive(flg, tinc, nxt, i, nT, lane);
                } else {
                    lab[i * 64 + lane] = (uint8_t)cur;
                    cur = nxt;
                    ex = ey;
                }
            }
            if (c + 1 == nchunks) lab[npairs * 64 + lane] = (uint8_t)cur;
        } else if (c + 1 < nchunks) {
            draw(c + 1, wave - 1, kPlanWaves - 1);
        }
        __syncthreads();
    }
    for (int t = wave; t < nT; t += kPlanWaves) {
        p.label[base + (size_t)t * 64] = lab[t * 64 + lane];
        p.flag[base + (size_t)t * 64] = flg[t * 64 + lane];
        if (tinc[t * 64 + lane]) p.trips[base + (size_t)t * 64] += 1;
    }
    if (valid) {
        const size_t pbase = (size_t)aw * npairs * 64 + lane;
        for (int i = wave; i < npairs; i += kPlanWaves) {
            p.att[pbase + (size_t)i * 64] += 1;
            if (accb[i * 64 + lane]) p.acc[pbase + (size_t)i * 64] += 1;
        }
    }
}

// grid (ceil(nsites / 256), A W): plane (t, a, w) lies at (t A W + a W + w) nsites.  Eight words of the column are loaded ahead of
// the eight exchanges that consume them, so the loads of a chunk are in flight together.
__global__ __launch_bounds__(256) void k9_pt_apply(uint64_t* __restrict__ s, const uint64_t* __restrict__ mask, int nT, int AW, int nsites) {
    constexpr int kAhead = 8;
    const int aw = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nsites) return;
    const long long stride = (long long)AW * nsites;
    uint64_t* x = s + (long long)aw * nsites + i;
    const uint64_t* m = mask + aw;
    uint64_t cur = x[0];
    for (int t0 = 0; t0 + 1 < nT; t0 += kAhead) {
        uint64_t nxt[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; ++k) nxt[k] = t0 + 1 + k < nT ? x[(long long)(t0 + 1 + k) * stride] : 0ull;
#pragma unroll
        for (int k = 0; k < kAhead; ++k)
            if (t0 + 1 + k < nT) {
                const uint64_t d = (cur ^ nxt[k]) & m[(long long)(t0 + k) * AW];
                x[(long long)(t0 + k) * stride] = cur ^ d;
                cur = nxt[k] ^ d;
            }
    }
    x[(long long)(nT - 1) * stride] = cur;
}

template <typename T>
hipError_t msc_pt_upload(T** dst, const std::vector<T>& src, hipStream_t st) {
    hipError_t e = hipMalloc((void**)dst, src.size() * sizeof(T));
    if (e == hipSuccess) e = hipMemcpyAsync(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // src may be a temporary
    return e;
}

}  // namespace

void msc_pt_free(tsu_msc* h) {
    msc_pt* pt = h->pt;
    if (!pt) return;
    void* bufs[] = {pt->d_dbeta, pt->d_skey, pt->d_mask, pt->d_label, pt->d_flag, pt->d_trips, pt->d_att, pt->d_acc, pt->d_hist};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    delete pt;
    h->pt = nullptr;
}

extern "C" {

int tsu_msc_pt_enable(tsu_msc* h, const double* T) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    TSU_REQUIRE(ctx, T, "msc_pt_enable: NULL input");
    TSU_REQUIRE(ctx, h->nT >= 2 && h->nT <= kMscPtMaxTemps, "msc_pt_enable: tempering needs 2 .. %d temperatures, got %d", kMscPtMaxTemps,
                h->nT);
    for (int t = 0; t < h->nT; ++t) TSU_REQUIRE(ctx, T[t] > 0.0 && std::isfinite(T[t]), "Temperature must be positive");
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    msc_pt_free(h);
    msc_pt* pt = new (std::nothrow) msc_pt();
    if (!pt) return tsu_fail(ctx, TSU_E_NOMEM, "msc_pt_enable: host allocation failed");
    h->pt = pt;
    const int nT = h->nT, AW = h->A * h->W;
    const size_t cols = (size_t)AW * nT * 64, pairs = (size_t)AW * (nT - 1) * 64;
    std::vector<uint8_t> label(cols), flag(cols, (uint8_t)kNone);
    for (int aw = 0; aw < AW; ++aw)
        for (int t = 0; t < nT; ++t)
            for (int b = 0; b < 64; ++b) {
                label[((size_t)aw * nT + t) * 64 + b] = (uint8_t)t;
                if (t == 0) flag[((size_t)aw * nT + t) * 64 + b] = (uint8_t)kBottom;
            }
    std::vector<double> dbeta((size_t)nT - 1);
    for (int i = 0; i + 1 < nT; ++i) dbeta[i] = 1.0 / T[i] - 1.0 / T[i + 1];
    hipError_t e = msc_pt_upload(&pt->d_dbeta, dbeta, ctx->stream);
    if (e == hipSuccess) e = msc_pt_upload(&pt->d_label, label, ctx->stream);
    if (e == hipSuccess) e = msc_pt_upload(&pt->d_flag, flag, ctx->stream);
    if (e == hipSuccess) e = msc_pt_upload(&pt->d_trips, std::vector<long long>(cols, 0), ctx->stream);
    if (e == hipSuccess) e = msc_pt_upload(&pt->d_att, std::vector<long long>(pairs, 0), ctx->stream);
    if (e == hipSuccess) e = msc_pt_upload(&pt->d_acc, std::vector<long long>(pairs, 0), ctx->stream);
    if (e == hipSuccess) e = msc_pt_upload(&pt->d_skey, std::vector<uint32_t>((size_t)h->W * 64 * 2, 0u), ctx->stream);
    if (e == hipSuccess) e = msc_pt_upload(&pt->d_mask, std::vector<uint64_t>((size_t)(nT - 1) * AW, 0ull), ctx->stream);
    if (e == hipSuccess) e = tsu_func_allow_lds(ctx, reinterpret_cast<const void*>(k9_pt_plan), (int)msc_pt_plan_lds(nT));
    if (e != hipSuccess) {
        const int rc = tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "msc_pt_enable: %s", hipGetErrorString(e));
        (void)hipStreamSynchronize(ctx->stream);
        msc_pt_free(h);
        return rc;
    }
    return TSU_OK;
}

int tsu_msc_pt_set_swap_seeds(tsu_msc* h, const uint64_t* seeds) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    TSU_REQUIRE(ctx, h->pt, "msc_pt_set_swap_seeds: call tsu_msc_pt_enable first");
    TSU_REQUIRE(ctx, seeds, "msc_pt_set_swap_seeds: NULL input");
    std::vector<uint32_t> key((size_t)h->W * 64 * 2, 0u);
    for (int s = 0; s < h->S; ++s) {
        key[2 * s] = (uint32_t)seeds[s];
        key[2 * s + 1] = (uint32_t)(seeds[s] >> 32);
    }
    TSU_HIP_TRY(ctx, hipMemcpyAsync(h->pt->d_skey, key.data(), key.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    h->pt->have_seeds = 1;
    return TSU_OK;
}

int tsu_msc_pt_run(tsu_msc* h, int n_rounds, int swap_interval, int do_swap, int record, uint32_t sweep0, uint32_t round0) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    msc_pt* pt = h->pt;
    TSU_REQUIRE(ctx, pt, "msc_pt_run: call tsu_msc_pt_enable first");
    TSU_REQUIRE(ctx, pt->have_seeds || !do_swap, "msc_pt_run: call tsu_msc_pt_set_swap_seeds first");
    TSU_REQUIRE(ctx, h->have_T && h->have_seeds, "msc_pt_run: call tsu_msc_set_temperatures and tsu_msc_set_seeds first");
    TSU_REQUIRE(ctx, n_rounds >= 0, "msc_pt_run: n_rounds must be >= 0");
    TSU_REQUIRE(ctx, swap_interval >= 0, "msc_pt_run: swap_interval must be >= 0");
    TSU_REQUIRE(ctx, (uint64_t)sweep0 + (uint64_t)n_rounds * (uint64_t)swap_interval <= (1ull << 31), "msc_pt_run: sweep counter overflow");
    TSU_REQUIRE(ctx, (uint64_t)round0 + (uint64_t)n_rounds <= (1ull << 32), "msc_pt_run: round counter overflow");
    const size_t row_len = msc_row_len(h);
    pt->hist_rows = 0;
    // rows on the device: the record's, one per round; without a record a ring of kScratchRows rows zeroed once per lap, so
    // that a round without a record costs no memset of its own (the contents mean nothing afterwards: hist_rows stays 0)
    const int ring = record ? n_rounds : (n_rounds < kScratchRows ? n_rounds : kScratchRows);
    if ((record || do_swap) && n_rounds > 0) {
        const size_t bytes = (size_t)ring * row_len * 8;
        if (pt->hist_cap < bytes) {
            TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            if (pt->d_hist) (void)hipFree(pt->d_hist);
            pt->d_hist = nullptr;
            pt->hist_cap = 0;
            TSU_HIP_TRY(ctx, hipMalloc((void**)&pt->d_hist, bytes));
            pt->hist_cap = bytes;
        }
        if (record) TSU_HIP_TRY(ctx, hipMemsetAsync(pt->d_hist, 0, bytes, ctx->stream));
    }
    const bool modes = msc_corr_on(h);  // off: every launch below is what it was without the correlation code
    if (modes) {
        const int rc = msc_corr_record_begin(h, record ? n_rounds : 0);
        if (rc != TSU_OK) return rc;
    }
    const int AW = h->A * h->W;
    MscPtPlan plan = {};
    plan.dbeta = pt->d_dbeta;
    plan.skey = pt->d_skey;
    plan.mask = pt->d_mask;
    plan.label = pt->d_label;
    plan.flag = pt->d_flag;
    plan.trips = pt->d_trips;
    plan.att = pt->d_att;
    plan.acc = pt->d_acc;
    plan.nb = msc_bonds(h->g);
    plan.nT = h->nT;
    plan.A = h->A;
    plan.W = h->W;
    plan.S = h->S;
    const dim3 apply_grid((unsigned)((h->g.nsites + 255) / 256), (unsigned)AW, 1);
    for (int r = 0; r < n_rounds; ++r) {
        const int rc = tsu_msc_sweep(h, swap_interval, sweep0 + (uint32_t)r * (uint32_t)swap_interval);
        if (rc != TSU_OK) return rc;
        if (!record && !do_swap) continue;
        if (!record && r % ring == 0) {
            const int lap = n_rounds - r < ring ? n_rounds - r : ring;
            TSU_HIP_TRY(ctx, hipMemsetAsync(pt->d_hist, 0, (size_t)lap * row_len * 8, ctx->stream));
        }
        unsigned long long* row = pt->d_hist + (size_t)(record ? r : r % ring) * row_len;
        TSU_HIP_TRY(ctx, msc_enqueue_measure(h, row));
        pt->launches += 1;
        if (record) pt->hist_rows = r + 1;
        if (record && modes) {  // before the pass: the modes of the configurations the row's q belongs to
            TSU_HIP_TRY(ctx, msc_corr_enqueue_row(h, r));
            pt->launches += kMscCorrLaunches;
        }
        if (!do_swap) continue;
        plan.row = row;
        plan.round = round0 + (uint32_t)r;
        k9_pt_plan<<<(unsigned)AW, 64 * kPlanWaves, msc_pt_plan_lds(h->nT), ctx->stream>>>(plan);
        k9_pt_apply<<<apply_grid, 256, 0, ctx->stream>>>(h->d_s, pt->d_mask, h->nT, AW, h->g.nsites);
        pt->launches += 2;
        TSU_HIP_TRY(ctx, hipGetLastError());
    }
    return TSU_OK;
}

int tsu_msc_pt_stats(tsu_msc* h, int64_t* attempts, int64_t* accepts, int32_t* labels, int32_t* flags, int64_t* trips) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    msc_pt* pt = h->pt;
    TSU_REQUIRE(ctx, pt, "msc_pt_stats: call tsu_msc_pt_enable first");
    TSU_REQUIRE(ctx, attempts && accepts && labels && flags && trips, "msc_pt_stats: NULL output");
    const int nT = h->nT, AW = h->A * h->W;
    const size_t cols = (size_t)AW * nT * 64, pairs = (size_t)AW * (nT - 1) * 64;
    std::vector<long long> att(pairs), acc(pairs), tr(cols);
    std::vector<uint8_t> lab(cols), flg(cols);
    TSU_HIP_TRY(ctx, hipMemcpyAsync(att.data(), pt->d_att, pairs * 8, hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipMemcpyAsync(acc.data(), pt->d_acc, pairs * 8, hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipMemcpyAsync(tr.data(), pt->d_trips, cols * 8, hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipMemcpyAsync(lab.data(), pt->d_label, cols, hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipMemcpyAsync(flg.data(), pt->d_flag, cols, hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int a = 0; a < h->A; ++a)
        for (int s = 0; s < h->S; ++s) {
            const size_t aw = (size_t)a * h->W + s / 64, b = s % 64, out = (size_t)a * h->S + s;
            for (int t = 0; t < nT; ++t) {
                const size_t at = (aw * nT + t) * 64 + b;
                labels[out * nT + t] = lab[at];
                flags[out * nT + t] = flg[at];
                trips[out * nT + t] = tr[at];
            }
            for (int i = 0; i + 1 < nT; ++i) {
                const size_t at = (aw * (nT - 1) + i) * 64 + b;
                attempts[out * (nT - 1) + i] = att[at];
                accepts[out * (nT - 1) + i] = acc[at];
            }
        }
    return TSU_OK;
}

int tsu_msc_pt_history(tsu_msc* h, int n_rows, int64_t* unsat, int64_t* sum, int64_t* q, int64_t* q_link) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    msc_pt* pt = h->pt;
    TSU_REQUIRE(ctx, pt, "msc_pt_history: call tsu_msc_pt_enable first");
    TSU_REQUIRE(ctx, n_rows == pt->hist_rows, "msc_pt_history: the last run recorded %d rounds, not %d", pt->hist_rows, n_rows);
    if (n_rows == 0) return TSU_OK;
    TSU_REQUIRE(ctx, unsat && sum, "msc_pt_history: NULL output");
    const size_t row_len = msc_row_len(h);
    const size_t col = (size_t)h->W * 64, n1 = (size_t)h->nT * h->A * col, nq = (size_t)h->nT * col;
    std::vector<unsigned long long> host((size_t)n_rows * row_len);
    TSU_HIP_TRY(ctx, hipMemcpyAsync(host.data(), pt->d_hist, host.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const long long N = h->g.nsites, nb = msc_bonds(h->g);
    for (int r = 0; r < n_rows; ++r) {
        const unsigned long long* row = host.data() + (size_t)r * row_len;
        for (size_t i = 0; i < n1; ++i) {
            unsat[(size_t)r * n1 + i] = (int64_t)row[i];
            sum[(size_t)r * n1 + i] = 2 * (int64_t)row[n1 + i] - N;
        }
        if (h->A == 2)
            for (size_t i = 0; i < nq; ++i) {
                if (q) q[(size_t)r * nq + i] = N - 2 * (int64_t)row[2 * n1 + i];
                if (q_link) q_link[(size_t)r * nq + i] = nb - 2 * (int64_t)row[2 * n1 + nq + i];
            }
    }
    return TSU_OK;
}

int tsu_msc_pt_launch_count(tsu_msc* h, uint64_t* out) {
    if (!h || !out || !h->pt) return TSU_E_INVALID;
    *out = h->pt->launches;
    return TSU_OK;
}

}  // extern "C"

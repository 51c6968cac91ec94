// multispin_corr.hip -- K9: axis profiles and k_min Fourier modes of a multispin-coded glass, 64 samples at once (gfx950).
//
// The site field is f = a b, the two replicas of a slot, or f = s with one replica (include/tsu_hip_multispin_corr.h, DESIGN.md
// section 3 "Correlation length of multispin-coded glasses (K9)").  In bits x = a ^ b (or ~a) has a set bit where f = -1, so the
// profile of axis d at coordinate c is P_d[c] = n_c - 2 count(bits set in x over the n_c = N / L_d sites with that coordinate):
// a positional popcount of one-bit planes, integers only.
//
// k9_profile: one launch for all (slot, word-plane) pairs (the grid's y) and all three axes.  A wave owns one unit = (axis d,
// coordinate c, part p): the sites j = p chunk .. of the n_c sites of that coordinate, lane l taking j0 + l, j0 + l + 64, ..., at most
// kProfileAdds = 255 of them into an 8-plane vertical counter (MscCount<8>), which therefore never overflows and is never flushed.
// The 64 lanes' counters are then added per sample bit without LDS: for counter plane k and bit b the wave's ballot of
// (cnt.b[k] >> b) & 1 is a lane mask, the scalar unit popcounts it and adds 2^k times that count over k, and lane b keeps the
// sum.  Planes k that are zero in every lane of the wave are left out (a 16^3 lattice has 4 sites per lane: 3 planes).  Lane b
// then holds sample 64 w + b's count and writes P with one store.  The host cuts a coordinate into parts only when it has more
// than 64 x 255 sites; then the parts add their shares with 32-bit integer atomics into scratch that a memset zeroed, otherwise
// (parts = 1 on every axis) there are no atomics and no zeroing.  No scratch memory, no LDS, no waiting on other workgroups, and
// no floating point of its own (the compiler's integer divisions aside).
//
// k9_modes: one wave per (slot, sample column, periodic axis), or a 2^n-lane segment of one when no periodic axis is longer than
// 32: F = sum_x P[x] (cos[x] + i sin[x]) from the host's tables in the contract's order.  Lane l keeps the partials l, l + 64,
// l + 128, l + 192 of the 256, each adding its terms x = t, t + 256, ... in ascending order from 0.0; the four groups fold by
// halves over lane shuffles at once, lane 0 adds (g0 + g1) + (g2 + g3).  Contraction is off: every product is rounded before its
// add, as NumPy rounds it.
#include <new>
#include <vector>

#include "multispin_host.h"

struct msc_corr {
    int32_t* d_prof;  // [slot][64 W][L_z + L_r + L_c] profiles, int32: |P| <= nsites < 2^31
    int enabled;
    int nper;         // periodic axes
    int off[3];       // where the axis's profile starts in a column's row of d_prof
    int parts[3];     // parts a coordinate of the axis is cut into
    int chunk[3];     // sites of a part (the last one may hold fewer)
    int units;        // waves of one (slot, word-plane): sum over axes of L_d parts_d
    int atomics;      // some axis has parts > 1: d_prof is zeroed before every profile launch
    double* d_tab;    // the host's tables: per periodic axis cos[L], sin[L]
    const double* cs[3];
    const double* sn[3];
    double* d_modes;  // [slot][64 W][nper][2]: tsu_msc_modes' own row
    double* d_rec;    // the record of the last tsu_msc_pt_run: rec_rows rows like d_modes
    size_t rec_cap;
    int rec_rows;
};

namespace {

constexpr int kProfileAdds = 255;  // additions of a lane into its MscCount<8>: 2^8 - 1, the most 8 planes hold
constexpr int kProfileWaves = 4;   // waves (units) of a workgroup
constexpr int kModeWaves = 4;

struct MscProf {
    const uint64_t* s;
    int32_t* out;
    int rows, cols, nsites;
    int W;
    int len[3], first[3], parts[3], chunk[3];  // first[d]: the axis's first unit
    int off[3];
    int ltot, units, atomics;
};

// The 64 lanes' counters added per sample bit, the low KM planes (the others are zero in every lane): for bit b the ballot of
// plane k's bit is a lane mask, its popcount times 2^k adds up on the scalar unit, and lane b keeps the sum.
template <int KM>
__device__ __forceinline__ int msc_wave_counts(const MscCount<8>& cnt, int lane) {
    int total = 0;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        uint32_t w[KM];
#pragma unroll
        for (int k = 0; k < KM; ++k) w[k] = half ? (uint32_t)(cnt.b[k] >> 32) : (uint32_t)cnt.b[k];
        for (int b = 0; b < 32; ++b) {
            const uint32_t bit = 1u << b;
            int n = 0;
#pragma unroll
            for (int k = 0; k < KM; ++k) n += __popcll(__ballot((w[k] & bit) != 0u)) << k;
            total = lane == 32 * half + b ? n : total;
        }
    }
    return total;
}

template <int A>
__global__ __launch_bounds__(64 * kProfileWaves) void k9_profile(MscProf p) {
    const int lane = threadIdx.x & 63;
    // wave-uniform by construction; the compiler is told so
    const int u = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kProfileWaves + (threadIdx.x >> 6)));
    if (u >= p.units) return;
    const int d = u >= p.first[2] ? 2 : (u >= p.first[1] ? 1 : 0);
    const int v = u - p.first[d];
    const int c = v / p.parts[d], part = v - c * p.parts[d];
    const int nc = p.nsites / p.len[d];
    const int j0 = part * p.chunk[d];
    const int j1 = min(nc, j0 + p.chunk[d]);  // chunk <= 64 kProfileAdds: at most kProfileAdds sites per lane
    const int t = blockIdx.y / p.W, w = blockIdx.y - t * p.W;
    const uint64_t* sa = p.s + (long long)((t * A) * p.W + w) * p.nsites;
    const uint64_t* sb = p.s + (long long)((t * A + A - 1) * p.W + w) * p.nsites;
    MscCount<8> cnt;
    cnt.clear();
    for (int j = j0 + lane; j < j1; j += 64) {
        int i;
        if (d == 0) {
            i = c * (p.rows * p.cols) + j;
        } else if (d == 1) {
            const int z = j / p.cols;
            i = (z * p.rows + c) * p.cols + (j - z * p.cols);
        } else {
            i = j * p.cols + c;
        }
        uint64_t x = sa[i];
        if constexpr (A == 2) x ^= sb[i];
        else x = ~x;
        cnt.add(x);  // a set bit: f = -1
    }
    int kmax = 0;  // counter planes in use anywhere in the wave
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (__ballot(cnt.b[k] != 0ull) != 0ull) kmax = k + 1;
    int total = 0;  // lane b: the set bits of sample 64 w + b
    switch (kmax) {
        case 1: total = msc_wave_counts<1>(cnt, lane); break;
        case 2: total = msc_wave_counts<2>(cnt, lane); break;
        case 3: total = msc_wave_counts<3>(cnt, lane); break;
        case 4: total = msc_wave_counts<4>(cnt, lane); break;
        case 5: total = msc_wave_counts<5>(cnt, lane); break;
        case 6: total = msc_wave_counts<6>(cnt, lane); break;
        case 7: total = msc_wave_counts<7>(cnt, lane); break;
        case 8: total = msc_wave_counts<8>(cnt, lane); break;
        default: break;
    }
    const int share = (j1 - j0) - 2 * total;
    int32_t* at = p.out + ((long long)(t * p.W + w) * 64 + lane) * p.ltot + p.off[d] + c;
    if (p.atomics) atomicAdd(at, share);
    else *at = share;
}

struct MscModes {
    const int32_t* prof;
    double* out;
    int ltot, n;         // n: periodic axes
    int seg;             // lanes of a unit: the power of two >= the longest periodic axis, at most 64
    int off[3], len[3];  // per periodic axis, in axis order
    const double* cs[3];
    const double* sn[3];
    long long units;     // slots x 64 W x n
};

// A unit is one (slot, sample column, periodic axis); it takes `seg` lanes, so a wave holds 64 / seg units when every periodic axis
// has at most 32 sites.  Lane sl of a unit keeps the partials sl + 64 g.  What is left out is exactly what adds +0.0 to a value
// that is not -0.0 (a partial starts at +0.0, so neither it nor a sum of partials is ever -0.0) and therefore changes no bit:
// the partials t >= L, the fold steps of width >= seg, and the groups g with 64 g >= L.
__global__ __launch_bounds__(64 * kModeWaves) void k9_modes(MscModes m) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int seg = m.seg, sl = lane & (seg - 1);
    const long long wave = (long long)blockIdx.x * kModeWaves + (threadIdx.x >> 6);
    const long long u = wave * (64 / seg) + lane / seg;
    const bool live = u < m.units;
    const long long col = live ? u / m.n : 0;
    const int k = live ? (int)(u - col * m.n) : 0;
    const int32_t* P = m.prof + col * m.ltot + m.off[k];
    const double* cs = m.cs[k];
    const double* sn = m.sn[k];
    const int L = live ? m.len[k] : 0;
    const int ng = seg < 64 ? 1 : (L + 63) >> 6;  // groups that hold a term; seg == 64: one unit per wave, L is wave-uniform
    double re[4], im[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        re[g] = 0.0;
        im[g] = 0.0;
        for (int x = sl + 64 * g; x < L; x += 256) {
            const double f = (double)P[x];
            const double pr = f * cs[x], pi = f * sn[x];
            re[g] = re[g] + pr;
            im[g] = im[g] + pi;
        }
    }
    for (int off = seg >> 1; off > 0; off >>= 1) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
            if (g < ng) {
                const double r = __shfl_down(re[g], off, 64), i = __shfl_down(im[g], off, 64);
                re[g] = re[g] + r;
                im[g] = im[g] + i;
            }
    }
    if (live && sl == 0) {
        m.out[2 * u] = (re[0] + re[1]) + (re[2] + re[3]);
        m.out[2 * u + 1] = (im[0] + im[1]) + (im[2] + im[3]);
    }
}

inline int msc_ltot(const tsu_msc* h) { return h->g.depth + h->g.rows + h->g.cols; }
inline size_t msc_cols(const tsu_msc* h) { return (size_t)h->nT * h->W * 64; }
inline size_t msc_mode_row(const tsu_msc* h) { return msc_cols(h) * h->corr->nper * 2; }

// the handle's correlation state with its profile scratch and the launch plan, made on first use
int msc_corr_state(tsu_msc* h, const char* who) {
    tsu_ctx* ctx = h->ctx;
    if (h->corr) return TSU_OK;
    msc_corr* c = new (std::nothrow) msc_corr();
    if (!c) return tsu_fail(ctx, TSU_E_NOMEM, "%s: host allocation failed", who);
    const int len[3] = {h->g.depth, h->g.rows, h->g.cols};
    int off = 0;
    for (int d = 0; d < 3; ++d) {
        const int nc = h->g.nsites / len[d];
        c->off[d] = off;
        off += len[d];
        c->parts[d] = (nc + 64 * kProfileAdds - 1) / (64 * kProfileAdds);
        c->chunk[d] = (nc + c->parts[d] - 1) / c->parts[d];
        c->units += len[d] * c->parts[d];
        if (c->parts[d] > 1) c->atomics = 1;
    }
    const hipError_t e = hipMalloc((void**)&c->d_prof, msc_cols(h) * msc_ltot(h) * sizeof(int32_t));
    if (e != hipSuccess) {
        delete c;
        return tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    h->corr = c;
    return TSU_OK;
}

hipError_t msc_enqueue_profile(tsu_msc* h) {
    const msc_corr* c = h->corr;
    MscProf p = {};
    p.s = h->d_s;
    p.out = c->d_prof;
    p.rows = h->g.rows;
    p.cols = h->g.cols;
    p.nsites = h->g.nsites;
    p.W = h->W;
    const int len[3] = {h->g.depth, h->g.rows, h->g.cols};
    int first = 0;
    for (int d = 0; d < 3; ++d) {
        p.len[d] = len[d];
        p.first[d] = first;
        p.parts[d] = c->parts[d];
        p.chunk[d] = c->chunk[d];
        p.off[d] = c->off[d];
        first += len[d] * c->parts[d];
    }
    p.ltot = msc_ltot(h);
    p.units = c->units;
    p.atomics = c->atomics;
    if (c->atomics) {
        const hipError_t e = hipMemsetAsync(c->d_prof, 0, msc_cols(h) * p.ltot * sizeof(int32_t), h->ctx->stream);
        if (e != hipSuccess) return e;
    }
    const dim3 grid((unsigned)((c->units + kProfileWaves - 1) / kProfileWaves), (unsigned)(h->nT * h->W), 1);
    if (h->A == 2) k9_profile<2><<<grid, 64 * kProfileWaves, 0, h->ctx->stream>>>(p);
    else k9_profile<1><<<grid, 64 * kProfileWaves, 0, h->ctx->stream>>>(p);
    return hipGetLastError();
}

// the profile launch and the mode launch into `row` (msc_mode_row doubles)
hipError_t msc_enqueue_modes(tsu_msc* h, double* row) {
    const msc_corr* c = h->corr;
    hipError_t e = msc_enqueue_profile(h);
    if (e != hipSuccess) return e;
    MscModes m = {};
    m.prof = c->d_prof;
    m.out = row;
    m.ltot = msc_ltot(h);
    m.n = c->nper;
    const int len[3] = {h->g.depth, h->g.rows, h->g.cols};
    int k = 0;
    for (int d = 0; d < 3; ++d)
        if (c->cs[d]) {
            m.off[k] = c->off[d];
            m.len[k] = len[d];
            m.cs[k] = c->cs[d];
            m.sn[k] = c->sn[d];
            ++k;
        }
    m.units = (long long)msc_cols(h) * c->nper;
    m.seg = 1;
    for (int a = 0; a < m.n; ++a)
        while (m.seg < 64 && m.seg < m.len[a]) m.seg <<= 1;
    const long long per_block = (long long)kModeWaves * (64 / m.seg);
    k9_modes<<<(unsigned)((m.units + per_block - 1) / per_block), 64 * kModeWaves, 0, h->ctx->stream>>>(m);
    return hipGetLastError();
}

}  // namespace

void msc_corr_free(tsu_msc* h) {
    msc_corr* c = h->corr;
    if (!c) return;
    void* bufs[] = {c->d_prof, c->d_tab, c->d_modes, c->d_rec};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    delete c;
    h->corr = nullptr;
}

int msc_corr_on(const tsu_msc* h) { return h->corr && h->corr->enabled; }

int msc_corr_record_begin(tsu_msc* h, int n_rows) {
    tsu_ctx* ctx = h->ctx;
    msc_corr* c = h->corr;
    c->rec_rows = 0;
    const size_t bytes = (size_t)n_rows * msc_mode_row(h) * sizeof(double);
    if (c->rec_cap < bytes) {
        TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (c->d_rec) (void)hipFree(c->d_rec);
        c->d_rec = nullptr;
        c->rec_cap = 0;
        TSU_HIP_TRY(ctx, hipMalloc((void**)&c->d_rec, bytes));
        c->rec_cap = bytes;
    }
    return TSU_OK;
}

hipError_t msc_corr_enqueue_row(tsu_msc* h, int r) {
    msc_corr* c = h->corr;
    const hipError_t e = msc_enqueue_modes(h, c->d_rec + (size_t)r * msc_mode_row(h));
    if (e == hipSuccess) c->rec_rows = r + 1;
    return e;
}

extern "C" {

int tsu_msc_profiles(tsu_msc* h, int64_t* p_z, int64_t* p_r, int64_t* p_c) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    TSU_REQUIRE(ctx, p_z && p_r && p_c, "msc_profiles: NULL output");
    const int rc = msc_corr_state(h, "msc_profiles");
    if (rc != TSU_OK) return rc;
    TSU_HIP_TRY(ctx, msc_enqueue_profile(h));
    const size_t cols = msc_cols(h), ltot = (size_t)msc_ltot(h);
    std::vector<int32_t> host(cols * ltot);
    TSU_HIP_TRY(ctx, hipMemcpyAsync(host.data(), h->corr->d_prof, host.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    int64_t* out[3] = {p_z, p_r, p_c};
    const int len[3] = {h->g.depth, h->g.rows, h->g.cols};
    for (size_t col = 0; col < cols; ++col)
        for (int d = 0; d < 3; ++d)
            for (int x = 0; x < len[d]; ++x) out[d][col * len[d] + x] = host[col * ltot + h->corr->off[d] + x];
    return TSU_OK;
}

int tsu_msc_set_correlation(tsu_msc* h, int enable, const double* cos_z, const double* sin_z, const double* cos_r, const double* sin_r,
                            const double* cos_c, const double* sin_c) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    if (!enable) {
        if (h->corr) {
            h->corr->enabled = 0;
            h->corr->rec_rows = 0;
        }
        return TSU_OK;
    }
    const double* cs[3] = {cos_z, cos_r, cos_c};
    const double* sn[3] = {sin_z, sin_r, sin_c};
    const int per[3] = {h->g.pz, h->g.pr, h->g.pc};
    const int len[3] = {h->g.depth, h->g.rows, h->g.cols};
    TSU_REQUIRE(ctx, per[0] + per[1] + per[2] > 0, "msc_set_correlation: the lattice has no periodic axis (no k_min mode is defined)");
    size_t n = 0;
    for (int d = 0; d < 3; ++d) {
        if (per[d]) {
            TSU_REQUIRE(ctx, cs[d] && sn[d], "msc_set_correlation: NULL table of periodic axis %d", d);
            n += 2 * (size_t)len[d];
        } else {
            TSU_REQUIRE(ctx, !cs[d] && !sn[d], "msc_set_correlation: axis %d is open: its tables must be NULL", d);
        }
    }
    const int rc = msc_corr_state(h, "msc_set_correlation");
    if (rc != TSU_OK) return rc;
    msc_corr* c = h->corr;
    c->enabled = 0;
    c->rec_rows = 0;
    c->nper = per[0] + per[1] + per[2];
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // a launch in flight may still read the old tables
    if (!c->d_tab) TSU_HIP_TRY(ctx, hipMalloc((void**)&c->d_tab, n * sizeof(double)));
    if (!c->d_modes) TSU_HIP_TRY(ctx, hipMalloc((void**)&c->d_modes, msc_mode_row(h) * sizeof(double)));
    std::vector<double> tab;
    tab.reserve(n);
    for (int d = 0; d < 3; ++d) {
        c->cs[d] = c->sn[d] = nullptr;
        if (!per[d]) continue;
        c->cs[d] = c->d_tab + tab.size();
        tab.insert(tab.end(), cs[d], cs[d] + len[d]);
        c->sn[d] = c->d_tab + tab.size();
        tab.insert(tab.end(), sn[d], sn[d] + len[d]);
    }
    TSU_HIP_TRY(ctx, hipMemcpyAsync(c->d_tab, tab.data(), n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    c->enabled = 1;
    return TSU_OK;
}

int tsu_msc_modes(tsu_msc* h, double* modes) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    TSU_REQUIRE(ctx, msc_corr_on(h), "msc_modes: call tsu_msc_set_correlation first");
    TSU_REQUIRE(ctx, modes, "msc_modes: NULL output");
    TSU_HIP_TRY(ctx, msc_enqueue_modes(h, h->corr->d_modes));
    TSU_HIP_TRY(ctx, hipMemcpyAsync(modes, h->corr->d_modes, msc_mode_row(h) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int tsu_msc_pt_history_modes(tsu_msc* h, int n_rows, double* modes) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    TSU_REQUIRE(ctx, msc_corr_on(h) && h->corr->rec_rows > 0,
                "msc_pt_history_modes: the last run recorded no modes (call tsu_msc_set_correlation before a recording run)");
    TSU_REQUIRE(ctx, n_rows == h->corr->rec_rows, "msc_pt_history_modes: the last run recorded %d rounds, not %d", h->corr->rec_rows, n_rows);
    TSU_REQUIRE(ctx, modes, "msc_pt_history_modes: NULL output");
    const size_t n = (size_t)n_rows * msc_mode_row(h);
    TSU_HIP_TRY(ctx, hipMemcpyAsync(modes, h->corr->d_rec, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

}  // extern "C"

// potts_muca.hip -- K11: multicanonical walkers of a q-state Potts lattice (include/tsu_hip_potts_muca.h, DESIGN.md sections 3 and 5).
//
// The acceptance of an update depends on the walker's total n_eq, so a walker's updates are sequential and the parallelism is
// across walkers: one lane follows one walker through every sweep of a call, and the state is laid out state[site][walker] (pitch
// wp = walkers rounded up to 64), so that a wave's accesses to one site of its 64 walkers are 64 contiguous bytes.  The site loop,
// the neighbour indices and the Philox counter words (i >> 1, t) are wave-uniform; the colours, n_eq, the colour counts N_c, the
// tunnel state and the table index are per lane and stay in registers for the whole call.
//
// k11_muca<STAGE, LOCAL>: STAGE keeps the workgroup's lattices in LDS (ls[site][thread]) for the call, LOCAL keeps the histogram
// (3 (B + 1) uint64) and the threshold table in LDS; without LOCAL the histogram takes global atomics and the table is gathered
// through L2.  The three routes are <1, 1>, <0, 1> and <0, 0>.
#include <stdlib.h>

#include <vector>

#include "potts_muca_dev.h"
#include "tsu_common.h"

struct tsu_potts_muca {
    tsu_ctx* ctx;
    MucaGeom g;
    int q;
    int walkers;
    long long wp;         // pitch of the state and of the per-walker arrays
    int8_t* d_s;          // state[site][walker]
    int32_t* d_n;         // n_eq per walker
    uint32_t* d_N;        // N_c: [8][wp]
    uint8_t* d_side;      // tunnel side per walker: 0 none, 1 low, 2 high
    uint32_t* d_tun;      // tunnel events per walker
    uint32_t* d_thr;      // min(thr, 2^32 - 1): (B + 1) (2 zmax + 1)
    uint16_t* d_alw;      // bit delta + zmax of word n: thr[n][delta] = 2^32
    unsigned long long* d_rec;  // H, S1, S2: 3 (B + 1)
    int* d_mismatch;      // k11_measure's flag
    int* h_err;           // host-mapped: a sweep found n_eq outside 0 .. B
    int n_lo, n_hi;
    unsigned long long launches;
};

namespace {

constexpr int kLdsCap = 160 * 1024;
constexpr int kSideLow = 1, kSideHigh = 2;

struct MucaParams {
    int8_t* s;
    long long wp;
    int walkers, q;
    MucaGeom g;
    int32_t* n;
    uint32_t* N;
    uint8_t* side;
    uint32_t* tun;
    const uint32_t* thr;
    const uint16_t* alw;
    unsigned long long* rec;
    int n_lo, n_hi;
    uint32_t k0, k1, tag, sweep0;
    int n_sweeps;
    int* err;
};

__host__ __device__ inline size_t muca_local_bytes(int bonds, int zmax) {
    const size_t b1 = (size_t)bonds + 1;
    return (b1 * (24 + 4 * (2 * zmax + 1) + 2) + 15) & ~(size_t)15;
}

// The colours of a lane's walker: LDS column `tid` of ls[site][T] or global column w of s[site][wp]
template <bool STAGE>
struct MucaSpins {
    int8_t* base;
    size_t pitch;
    __device__ __forceinline__ int get(int i) const { return base[(size_t)i * pitch]; }
    __device__ __forceinline__ void put(int i, int c) const { base[(size_t)i * pitch] = (int8_t)c; }
};

struct MucaWalker {
    int n;
    uint32_t N[8];
};

// One update of site i = (z, r, c) (all wave-uniform) of the lane's walker with proposal word P and uniform u
template <bool STAGE>
__device__ __forceinline__ void muca_site(const MucaParams& p, const MucaSpins<STAGE>& sp, const uint32_t* thr, const uint16_t* alw,
                                          MucaWalker& wk, int i, int z, int r, int c, uint32_t P, uint32_t u) {
    const MucaGeom& g = p.g;
    const int plane = g.rows * g.cols;
    const int cur = sp.get(i);
    int cn = cur + 1 + (int)__umulhi(P, (uint32_t)(p.q - 1));
    if (cn >= p.q) cn -= p.q;
    int d = 0;
    auto nb = [&](int j) {
        const int v = sp.get(j);
        d += (int)(v == cn) - (int)(v == cur);
    };
    if (c > 0) nb(i - 1);
    else if (g.pc && g.cols >= 2) nb(i + g.cols - 1);
    if (c < g.cols - 1) nb(i + 1);
    else if (g.pc && g.cols >= 2) nb(i - (g.cols - 1));
    if (r > 0) nb(i - g.cols);
    else if (g.pr && g.rows >= 2) nb(i + plane - g.cols);
    if (r < g.rows - 1) nb(i + g.cols);
    else if (g.pr && g.rows >= 2) nb(i - (plane - g.cols));
    if (z > 0) nb(i - plane);
    else if (g.pz && g.depth >= 2) nb(i + g.sites - plane);
    if (z < g.depth - 1) nb(i + plane);
    else if (g.pz && g.depth >= 2) nb(i - (g.sites - plane));
    const int K = 2 * g.zmax + 1;
    const uint32_t lo = thr[wk.n * K + d + g.zmax];
    const uint32_t always = ((uint32_t)alw[wk.n] >> (d + g.zmax)) & 1u;
    if ((u < lo) | (always != 0)) {
        sp.put(i, cn);
        wk.n += d;
#pragma unroll
        for (int k = 0; k < 8; ++k) wk.N[k] += (uint32_t)(k == cn) - (uint32_t)(k == cur);
    }
}

template <bool STAGE, bool LOCAL>
__global__ __launch_bounds__(1024) void k11_muca(MucaParams p) {
    extern __shared__ __align__(16) unsigned char lds[];
    const MucaGeom& g = p.g;
    const int T = (int)blockDim.x, tid = (int)threadIdx.x;
    const int b1 = g.bonds + 1, K = 2 * g.zmax + 1;
    const long long w = (long long)blockIdx.x * T + tid;
    const bool active = w < p.walkers;
    unsigned long long* hist = reinterpret_cast<unsigned long long*>(lds);
    uint32_t* lthr = reinterpret_cast<uint32_t*>(lds + (size_t)24 * b1);
    uint16_t* lalw = reinterpret_cast<uint16_t*>(lds + (size_t)24 * b1 + (size_t)4 * b1 * K);
    int8_t* ls = reinterpret_cast<int8_t*>(lds + muca_local_bytes(g.bonds, g.zmax));
    if (LOCAL) {
        for (int b = tid; b < 3 * b1; b += T) hist[b] = 0ull;
        for (int b = tid; b < b1 * K; b += T) lthr[b] = p.thr[b];
        for (int b = tid; b < b1; b += T) lalw[b] = p.alw[b];
    }
    if (STAGE && active)
        for (int i = 0; i < g.sites; ++i) ls[(size_t)i * T + tid] = p.s[(size_t)i * p.wp + w];
    if (LOCAL) __syncthreads();
    if (active) {
        const MucaSpins<STAGE> sp = STAGE ? MucaSpins<STAGE>{ls + tid, (size_t)T} : MucaSpins<STAGE>{p.s + w, (size_t)p.wp};
        const uint32_t* thr = LOCAL ? lthr : p.thr;
        const uint16_t* alw = LOCAL ? lalw : p.alw;
        MucaWalker wk;
        wk.n = p.n[w];
#pragma unroll
        for (int k = 0; k < 8; ++k) wk.N[k] = p.N[(size_t)k * p.wp + w];
        int side = p.side[w];
        uint32_t tun = p.tun[w];
        for (int k = 0; k < p.n_sweeps; ++k) {
            const uint32_t t = p.sweep0 + (uint32_t)k;
            int z = 0, r = 0, c = 0;
            for (int i = 0; i < g.sites; i += 2) {
                const u32x4 x = tsu_philox((uint32_t)(i >> 1), (uint32_t)w, t, p.tag, p.k0, p.k1);
                muca_site<STAGE>(p, sp, thr, alw, wk, i, z, r, c, x.x, x.y);
                if (++c == g.cols) {
                    c = 0;
                    if (++r == g.rows) {
                        r = 0;
                        ++z;
                    }
                }
                if (i + 1 < g.sites) {
                    muca_site<STAGE>(p, sp, thr, alw, wk, i + 1, z, r, c, x.z, x.w);
                    if (++c == g.cols) {
                        c = 0;
                        if (++r == g.rows) {
                            r = 0;
                            ++z;
                        }
                    }
                }
            }
            if ((unsigned)wk.n > (unsigned)g.bonds) {  // cannot happen with a state k11_measure counted: no index is formed from it
                *p.err = 1;
                break;
            }
            uint32_t nmax = wk.N[0];
#pragma unroll
            for (int j = 1; j < 8; ++j) nmax = wk.N[j] > nmax ? wk.N[j] : nmax;
            unsigned long long* rec = LOCAL ? hist : p.rec;
            atomicAdd(&rec[wk.n], 1ull);
            atomicAdd(&rec[b1 + wk.n], (unsigned long long)nmax);
            atomicAdd(&rec[2 * b1 + wk.n], (unsigned long long)nmax * nmax);
            if (wk.n <= p.n_lo) {
                tun += (uint32_t)(side == kSideHigh);
                side = kSideLow;
            } else if (wk.n >= p.n_hi) {
                tun += (uint32_t)(side == kSideLow);
                side = kSideHigh;
            }
        }
        p.n[w] = wk.n;
#pragma unroll
        for (int k = 0; k < 8; ++k) p.N[(size_t)k * p.wp + w] = wk.N[k];
        p.side[w] = (uint8_t)side;
        p.tun[w] = tun;
        if (STAGE)
            for (int i = 0; i < g.sites; ++i) p.s[(size_t)i * p.wp + w] = ls[(size_t)i * T + tid];
    }
    if (LOCAL) {
        __syncthreads();
        for (int b = tid; b < 3 * b1; b += T) {
            const unsigned long long v = hist[b];
            if (v) atomicAdd(&p.rec[b], v);
        }
    }
}

// n_eq and N_c of every walker from its colours, one lane per walker; check != 0: raise *mismatch where they differ from the kept ones
__global__ __launch_bounds__(256) void k11_measure(MucaParams p, int check, int* mismatch) {
    const MucaGeom& g = p.g;
    const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
    if (w >= p.walkers) return;
    const int8_t* s = p.s + w;
    const int plane = g.rows * g.cols;
    int n = 0;
    uint32_t N[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int z = 0, r = 0, c = 0;
    for (int i = 0; i < g.sites; ++i) {
        const int v = s[(size_t)i * p.wp];
#pragma unroll
        for (int k = 0; k < 8; ++k) N[k] += (uint32_t)(k == v);
        if (c < g.cols - 1) n += (int)(s[(size_t)(i + 1) * p.wp] == v);
        else if (g.pc && g.cols >= 2) n += (int)(s[(size_t)(i - (g.cols - 1)) * p.wp] == v);
        if (r < g.rows - 1) n += (int)(s[(size_t)(i + g.cols) * p.wp] == v);
        else if (g.pr && g.rows >= 2) n += (int)(s[(size_t)(i - (plane - g.cols)) * p.wp] == v);
        if (z < g.depth - 1) n += (int)(s[(size_t)(i + plane) * p.wp] == v);
        else if (g.pz && g.depth >= 2) n += (int)(s[(size_t)(i - (g.sites - plane)) * p.wp] == v);
        if (++c == g.cols) {
            c = 0;
            if (++r == g.rows) {
                r = 0;
                ++z;
            }
        }
    }
    bool same = p.n[w] == n;
#pragma unroll
    for (int k = 0; k < 8; ++k) same = same && p.N[(size_t)k * p.wp + w] == N[k];
    if (check && !same) *mismatch = 1;
    p.n[w] = n;
#pragma unroll
    for (int k = 0; k < 8; ++k) p.N[(size_t)k * p.wp + w] = N[k];
}

// ---------------------------------------------------------------- host side
struct MucaPlan {
    int route;
    int threads;
    size_t lds;
};

int env_int(const char* name, int none) {
    const char* e = getenv(name);
    return (e && *e) ? atoi(e) : none;
}

// 256 walkers a workgroup where the LDS allows, else 128, else 64: measured (profiles/potts_muca_time.txt), 256 is the best or within
// 2 % of it on every route (64 costs half the rate on the LDS route at 16 x 16, 1024 a tenth or more on the others), also where
// that leaves CUs without a workgroup.  TSU_POTTS_MUCA_BLOCK overrides it where the LDS allows.
int muca_threads(const tsu_potts_muca* M, size_t fixed, size_t per_thread) {
    const int forced = env_int("TSU_POTTS_MUCA_BLOCK", 0);
    if (forced >= 64 && forced <= 1024 && forced % 64 == 0 && fixed + per_thread * (size_t)forced <= (size_t)kLdsCap) return forced;
    for (int T = 256; T > 64; T >>= 1)
        if (fixed + per_thread * (size_t)T <= (size_t)kLdsCap && M->walkers > T / 2) return T;
    return 64;
}

MucaPlan plan_of(const tsu_potts_muca* M) {
    const size_t local = muca_local_bytes(M->g.bonds, M->g.zmax);
    int route = TSU_POTTS_MUCA_ROUTE_ATOMICS;
    if (local + (size_t)M->g.sites * 64 <= (size_t)kLdsCap) route = TSU_POTTS_MUCA_ROUTE_LDS;
    else if (local <= (size_t)kLdsCap) route = TSU_POTTS_MUCA_ROUTE_GLOBAL;
    const int forced = env_int("TSU_POTTS_MUCA_ROUTE", -1);  // tests, read per call: towards the more general route only
    if (forced > route && forced <= TSU_POTTS_MUCA_ROUTE_ATOMICS) route = forced;
    MucaPlan pl;
    pl.route = route;
    if (route == TSU_POTTS_MUCA_ROUTE_LDS) {
        pl.threads = muca_threads(M, local, (size_t)M->g.sites);
        pl.lds = local + (size_t)M->g.sites * pl.threads;
    } else if (route == TSU_POTTS_MUCA_ROUTE_GLOBAL) {
        pl.threads = muca_threads(M, local, 0);
        pl.lds = local;
    } else {
        pl.threads = muca_threads(M, 0, 0);
        pl.lds = 0;
    }
    return pl;
}

MucaParams params_of(tsu_potts_muca* M) {
    MucaParams p = {};
    p.s = M->d_s;
    p.wp = M->wp;
    p.walkers = M->walkers;
    p.q = M->q;
    p.g = M->g;
    p.n = M->d_n;
    p.N = M->d_N;
    p.side = M->d_side;
    p.tun = M->d_tun;
    p.thr = M->d_thr;
    p.alw = M->d_alw;
    p.rec = M->d_rec;
    p.n_lo = M->n_lo;
    p.n_hi = M->n_hi;
    return p;
}

int check_err(tsu_potts_muca* M) {
    if (M->h_err && *M->h_err) {
        *M->h_err = 0;
        return tsu_fail(M->ctx, TSU_E_HIP, "potts_muca: a walker's n_eq left 0 .. B; results invalid");
    }
    return TSU_OK;
}

// n_eq and N_c of every walker from the colours; *equal (may be NULL): whether they were the kept ones.  Synchronises.
int measure(tsu_potts_muca* M, int* equal) {
    tsu_ctx* ctx = M->ctx;
    TSU_HIP_TRY(ctx, hipMemsetAsync(M->d_mismatch, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k11_measure, dim3((unsigned)((M->walkers + 255) / 256)), dim3(256), 0, ctx->stream, params_of(M), equal ? 1 : 0, M->d_mismatch);
    TSU_HIP_TRY(ctx, hipGetLastError());
    int bad = 0;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(&bad, M->d_mismatch, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (equal) *equal = bad ? 0 : 1;
    return check_err(M);
}

int upload_weights(tsu_potts_muca* M, const double* lnw) {
    tsu_ctx* ctx = M->ctx;
    const size_t b1 = (size_t)M->g.bonds + 1, K = 2 * (size_t)M->g.zmax + 1;
    std::vector<uint64_t> thr(b1 * K);
    muca_thresholds(M->g.bonds, M->g.zmax, lnw, thr.data());
    std::vector<uint32_t> lo(b1 * K);
    std::vector<uint16_t> alw(b1, 0);
    for (size_t n = 0; n < b1; ++n)
        for (size_t d = 0; d < K; ++d) {
            const uint64_t t = thr[n * K + d];
            lo[n * K + d] = t >> 32 ? 0xFFFFFFFFu : (uint32_t)t;
            if (t >> 32) alw[n] = (uint16_t)(alw[n] | (1u << d));
        }
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // a run in flight still reads the old table
    TSU_HIP_TRY(ctx, hipMemcpy(M->d_thr, lo.data(), lo.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    TSU_HIP_TRY(ctx, hipMemcpy(M->d_alw, alw.data(), alw.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    return TSU_OK;
}

void free_all(tsu_potts_muca* M) {
    if (M->d_s) (void)hipFree(M->d_s);
    if (M->d_n) (void)hipFree(M->d_n);
    if (M->d_N) (void)hipFree(M->d_N);
    if (M->d_side) (void)hipFree(M->d_side);
    if (M->d_tun) (void)hipFree(M->d_tun);
    if (M->d_thr) (void)hipFree(M->d_thr);
    if (M->d_alw) (void)hipFree(M->d_alw);
    if (M->d_rec) (void)hipFree(M->d_rec);
    if (M->d_mismatch) (void)hipFree(M->d_mismatch);
    if (M->h_err) (void)hipHostFree(M->h_err);
    delete M;
}

template <bool STAGE, bool LOCAL>
int launch(tsu_potts_muca* M, const MucaPlan& pl, MucaParams& p) {
    tsu_ctx* ctx = M->ctx;
    const void* fn = reinterpret_cast<const void*>(k11_muca<STAGE, LOCAL>);
    if (pl.lds > 64 * 1024) TSU_HIP_TRY(ctx, tsu_func_allow_lds(ctx, fn, kLdsCap));
    hipLaunchKernelGGL((k11_muca<STAGE, LOCAL>), dim3((unsigned)((M->walkers + pl.threads - 1) / pl.threads)), dim3((unsigned)pl.threads), pl.lds,
                       ctx->stream, p);
    TSU_HIP_TRY(ctx, hipGetLastError());
    return TSU_OK;
}

}  // namespace

extern "C" {

int tsu_potts_muca_geometry(int depth, int rows, int cols, const int* periodic, int64_t* bonds, int* z_max) {
    MucaGeom g;
    if (!periodic || !bonds || !z_max) return TSU_E_INVALID;
    if (!muca_geometry(depth, rows, cols, periodic[0], periodic[1], periodic[2], TSU_POTTS_MUCA_MAX_SITES, &g)) return TSU_E_INVALID;
    *bonds = g.bonds;
    *z_max = g.zmax;
    return TSU_OK;
}

int tsu_potts_muca_thresholds(int64_t bonds, int z_max, const double* lnw, uint64_t* out) {
    if (bonds < 0 || bonds > 3ll * TSU_POTTS_MUCA_MAX_SITES || (z_max != 4 && z_max != 6) || !lnw || !out) return TSU_E_INVALID;
    for (int64_t n = 0; n <= bonds; ++n)
        if (!isfinite(lnw[n])) return TSU_E_INVALID;
    muca_thresholds(bonds, z_max, lnw, out);
    return TSU_OK;
}

int tsu_potts_muca_create(tsu_ctx* ctx, int depth, int rows, int cols, int q, const int* periodic, int walkers, tsu_potts_muca** out) {
    TSU_ENTER(ctx);
    if (!ctx || !out) return TSU_E_INVALID;
    TSU_REQUIRE(ctx, periodic, "potts_muca_create: periodic is NULL");
    TSU_REQUIRE(ctx, q >= 2 && q <= 8, "potts_muca_create: q must be in 2 .. 8 (got %d)", q);
    TSU_REQUIRE(ctx, depth >= 1 && rows >= 1 && cols >= 1, "potts_muca_create: depth, rows and cols must be >= 1");
    MucaGeom g;
    TSU_REQUIRE(ctx, muca_geometry(depth, rows, cols, periodic[0], periodic[1], periodic[2], TSU_POTTS_MUCA_MAX_SITES, &g),
                "potts_muca_create: more than %d sites", TSU_POTTS_MUCA_MAX_SITES);
    TSU_REQUIRE(ctx, walkers >= 1 && walkers <= TSU_POTTS_MUCA_MAX_WALKERS, "potts_muca_create: walkers must be in 1 .. 2^20 (got %d)", walkers);
    TSU_REQUIRE(ctx, (long long)walkers * g.sites <= 2147483647ll, "potts_muca_create: walkers * sites exceeds 2^31 - 1");
    tsu_potts_muca* M = new tsu_potts_muca();
    M->ctx = ctx;
    M->g = g;
    M->q = q;
    M->walkers = walkers;
    M->wp = ((long long)walkers + 63) & ~63ll;
    M->n_lo = 0;
    M->n_hi = g.bonds > 0 ? g.bonds : 1;
    const size_t wp = (size_t)M->wp, b1 = (size_t)g.bonds + 1, K = 2 * (size_t)g.zmax + 1;
    hipError_t e = hipMalloc((void**)&M->d_s, (size_t)g.sites * wp);
    if (e == hipSuccess) e = hipMalloc((void**)&M->d_n, wp * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&M->d_N, 8 * wp * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&M->d_side, wp);
    if (e == hipSuccess) e = hipMalloc((void**)&M->d_tun, wp * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&M->d_thr, b1 * K * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&M->d_alw, b1 * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMalloc((void**)&M->d_rec, 3 * b1 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void**)&M->d_mismatch, sizeof(int));
    if (e == hipSuccess) e = hipMemsetAsync(M->d_s, 0, (size_t)g.sites * wp, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(M->d_n, 0, wp * sizeof(int32_t), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(M->d_N, 0, 8 * wp * sizeof(uint32_t), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(M->d_side, 0, wp, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(M->d_tun, 0, wp * sizeof(uint32_t), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(M->d_rec, 0, 3 * b1 * sizeof(unsigned long long), ctx->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        free_all(M);
        return tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "potts_muca_create: %s", hipGetErrorString(e));
    }
    int* d_err = nullptr;
    int rc = tsu_err_flag(ctx, M->h_err, &d_err);
    if (rc == TSU_OK) {
        const std::vector<double> zero(b1, 0.0);
        rc = upload_weights(M, zero.data());
    }
    if (rc == TSU_OK) rc = measure(M, nullptr);
    if (rc != TSU_OK) {
        free_all(M);
        return rc;
    }
    *out = M;
    return TSU_OK;
}

int tsu_potts_muca_destroy(tsu_potts_muca* M) {
    TSU_ENTER(M ? M->ctx : nullptr);
    if (!M) return TSU_E_INVALID;
    (void)hipStreamSynchronize(M->ctx->stream);
    free_all(M);
    return TSU_OK;
}

int tsu_potts_muca_set_weights(tsu_potts_muca* M, const double* lnw, int64_t len) {
    TSU_ENTER(M ? M->ctx : nullptr);
    if (!M) return TSU_E_INVALID;
    tsu_ctx* ctx = M->ctx;
    TSU_REQUIRE(ctx, lnw, "potts_muca_set_weights: lnw is NULL");
    TSU_REQUIRE(ctx, len == (int64_t)M->g.bonds + 1, "potts_muca_set_weights: %lld weights for B + 1 = %d levels", (long long)len, M->g.bonds + 1);
    for (int64_t n = 0; n < len; ++n) TSU_REQUIRE(ctx, isfinite(lnw[n]), "potts_muca_set_weights: ln W[%lld] is not finite", (long long)n);
    return upload_weights(M, lnw);
}

int tsu_potts_muca_set_spins(tsu_potts_muca* M, const int8_t* colours) {
    TSU_ENTER(M ? M->ctx : nullptr);
    if (!M) return TSU_E_INVALID;
    tsu_ctx* ctx = M->ctx;
    TSU_REQUIRE(ctx, colours, "potts_muca_set_spins: colours is NULL");
    const size_t sites = (size_t)M->g.sites, W = (size_t)M->walkers, wp = (size_t)M->wp;
    for (size_t k = 0; k < W * sites; ++k)
        TSU_REQUIRE(ctx, colours[k] >= 0 && colours[k] < M->q, "potts_muca_set_spins: colour %d of walker %zu, site %zu is outside 0 .. %d",
                    (int)colours[k], k / sites, k % sites, M->q - 1);
    std::vector<int8_t> t(sites * wp, 0);
    for (size_t w = 0; w < W; ++w)
        for (size_t i = 0; i < sites; ++i) t[i * wp + w] = colours[w * sites + i];
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    TSU_HIP_TRY(ctx, hipMemcpy(M->d_s, t.data(), t.size(), hipMemcpyHostToDevice));
    return measure(M, nullptr);
}

int tsu_potts_muca_get_spins(tsu_potts_muca* M, int8_t* colours) {
    TSU_ENTER(M ? M->ctx : nullptr);
    if (!M) return TSU_E_INVALID;
    tsu_ctx* ctx = M->ctx;
    TSU_REQUIRE(ctx, colours, "potts_muca_get_spins: colours is NULL");
    const size_t sites = (size_t)M->g.sites, W = (size_t)M->walkers, wp = (size_t)M->wp;
    std::vector<int8_t> t(sites * wp);
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    TSU_HIP_TRY(ctx, hipMemcpy(t.data(), M->d_s, t.size(), hipMemcpyDeviceToHost));
    for (size_t w = 0; w < W; ++w)
        for (size_t i = 0; i < sites; ++i) colours[w * sites + i] = t[i * wp + w];
    return check_err(M);
}

int tsu_potts_muca_fill(tsu_potts_muca* M, int colour) {
    TSU_ENTER(M ? M->ctx : nullptr);
    if (!M) return TSU_E_INVALID;
    tsu_ctx* ctx = M->ctx;
    TSU_REQUIRE(ctx, colour >= 0 && colour < M->q, "potts_muca_fill: colour %d is outside 0 .. %d", colour, M->q - 1);
    TSU_HIP_TRY(ctx, hipMemsetAsync(M->d_s, colour, (size_t)M->g.sites * (size_t)M->wp, ctx->stream));
    return measure(M, nullptr);
}

int tsu_potts_muca_set_tunnel_bounds(tsu_potts_muca* M, int64_t n_lo, int64_t n_hi) {
    TSU_ENTER(M ? M->ctx : nullptr);
    if (!M) return TSU_E_INVALID;
    tsu_ctx* ctx = M->ctx;
    TSU_REQUIRE(ctx, n_lo >= 0 && n_lo < n_hi && n_hi <= (M->g.bonds > 0 ? M->g.bonds : 1),
                "potts_muca_set_tunnel_bounds: need 0 <= n_lo < n_hi <= B (got %lld, %lld)", (long long)n_lo, (long long)n_hi);
    M->n_lo = (int)n_lo;
    M->n_hi = (int)n_hi;
    TSU_HIP_TRY(ctx, hipMemsetAsync(M->d_side, 0, (size_t)M->wp, ctx->stream));
    TSU_HIP_TRY(ctx, hipMemsetAsync(M->d_tun, 0, (size_t)M->wp * sizeof(uint32_t), ctx->stream));
    return TSU_OK;
}

int tsu_potts_muca_run(tsu_potts_muca* M, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica) {
    TSU_ENTER(M ? M->ctx : nullptr);
    if (!M) return TSU_E_INVALID;
    tsu_ctx* ctx = M->ctx;
    TSU_REQUIRE(ctx, n_sweeps >= 0, "potts_muca_run: n_sweeps must be >= 0");
    TSU_REQUIRE_REPLICA(ctx, replica, "potts_muca_run");
    if (n_sweeps == 0) return TSU_OK;
    const MucaPlan pl = plan_of(M);
    MucaParams p = params_of(M);
    p.k0 = (uint32_t)seed;
    p.k1 = (uint32_t)(seed >> 32);
    p.tag = TSU_TAG_POTTS_MUCA | (replica << 8);
    p.sweep0 = sweep0;
    p.n_sweeps = n_sweeps;
    int rc = tsu_err_flag(ctx, M->h_err, &p.err);
    if (rc != TSU_OK) return rc;
    if (pl.route == TSU_POTTS_MUCA_ROUTE_LDS) rc = launch<true, true>(M, pl, p);
    else if (pl.route == TSU_POTTS_MUCA_ROUTE_GLOBAL) rc = launch<false, true>(M, pl, p);
    else rc = launch<false, false>(M, pl, p);
    if (rc == TSU_OK) M->launches += 1;
    return rc;
}

int tsu_potts_muca_energies(tsu_potts_muca* M, int32_t* n_eq) {
    TSU_ENTER(M ? M->ctx : nullptr);
    if (!M) return TSU_E_INVALID;
    tsu_ctx* ctx = M->ctx;
    TSU_REQUIRE(ctx, n_eq, "potts_muca_energies: n_eq is NULL");
    TSU_HIP_TRY(ctx, hipMemcpyAsync(n_eq, M->d_n, (size_t)M->walkers * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return check_err(M);
}

int tsu_potts_muca_tunnels(tsu_potts_muca* M, uint32_t* events) {
    TSU_ENTER(M ? M->ctx : nullptr);
    if (!M) return TSU_E_INVALID;
    tsu_ctx* ctx = M->ctx;
    TSU_REQUIRE(ctx, events, "potts_muca_tunnels: events is NULL");
    TSU_HIP_TRY(ctx, hipMemcpyAsync(events, M->d_tun, (size_t)M->walkers * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return check_err(M);
}

int tsu_potts_muca_record(tsu_potts_muca* M, uint64_t* H, uint64_t* S1, uint64_t* S2) {
    TSU_ENTER(M ? M->ctx : nullptr);
    if (!M) return TSU_E_INVALID;
    tsu_ctx* ctx = M->ctx;
    const size_t b1 = (size_t)M->g.bonds + 1;
    uint64_t* out[3] = {H, S1, S2};
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 3; ++k)
        if (out[k]) TSU_HIP_TRY(ctx, hipMemcpy(out[k], M->d_rec + (size_t)k * b1, b1 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return check_err(M);
}

int tsu_potts_muca_clear_record(tsu_potts_muca* M) {
    TSU_ENTER(M ? M->ctx : nullptr);
    if (!M) return TSU_E_INVALID;
    TSU_HIP_TRY(M->ctx, hipMemsetAsync(M->d_rec, 0, 3 * ((size_t)M->g.bonds + 1) * sizeof(unsigned long long), M->ctx->stream));
    return TSU_OK;
}

int tsu_potts_muca_measure(tsu_potts_muca* M, int* equal) {
    TSU_ENTER(M ? M->ctx : nullptr);
    if (!M) return TSU_E_INVALID;
    TSU_REQUIRE(M->ctx, equal, "potts_muca_measure: equal is NULL");
    return measure(M, equal);
}

int tsu_potts_muca_route(tsu_potts_muca* M, int* route) {
    TSU_ENTER(M ? M->ctx : nullptr);
    if (!M || !route) return TSU_E_INVALID;
    *route = plan_of(M).route;
    return TSU_OK;
}

int tsu_potts_muca_launch_count(tsu_potts_muca* M, uint64_t* n) {
    TSU_ENTER(M ? M->ctx : nullptr);
    if (!M || !n) return TSU_E_INVALID;
    *n = M->launches;
    return TSU_OK;
}

}  // extern "C"

// multispin.hip -- K9: multispin-coded heat-bath sweeps of the bimodal (J = +-1, zero field) Edwards-Anderson glass (gfx950).
//
// 64 disorder samples share one 64-bit word per site: bit b of word-plane w is sample 64 w + b, a set bit is spin +1, a set coupling
// bit is J = -1 (include/tsu_hip_multispin.h, DESIGN.md section 3 "Multispin coding (K9)").  Every bit-plane is the chain K8 runs on
// that sample with the plane's seed: the same colours, half-sweeps, site uniforms and rule u < thr(f).  The 64 samples of a word share
// the site's uniform, so one Philox block serves 8 sites x 64 samples, and the threshold is one of 13 table entries per slot.
//
// The planes lie in the canonical order the ABI hands over: plane p = (t A + a) W + w, word (z, r, c) at ((z R + r) C + c).
//
// k9_sweep (the HBM route): one launch per half-sweep for all planes, the plane is the grid's z dimension.  A wave takes 64
// consecutive octets (z R + r, q) = 64 Philox blocks, lane l computes the block of octet l once, and in step i = 0 .. 7 the wave
// updates octets 8 i .. 8 i + 7: lane l takes site m = l & 7 of octet 8 i + (l >> 3) and fetches that octet's block and
// coordinates from lane 8 i + (l >> 3) by lane permutes.  So a Philox block is computed once for its 8 sites, and the 8 lanes of an
// octet read 8 of 16 consecutive words (the colour's), consecutive octets of a row follow each other.  In place: a colour reads only
// the other colour.  No scratch, no atomics, no waiting on other workgroups.
//
// k9_small: planes of at most 8192 sites (64 KiB of spins) with at most 1024 octets.  One workgroup of 1024 lanes per plane, the spins
// stay in LDS for all sweeps of a call, couplings come through L2.  The Philox blocks of four half-sweeps are computed ahead into LDS
// by all lanes (one block per lane and step), then each half-sweep is one pass of one lane per site with a barrier behind it.  The
// site update is k9_sweep's (msc_site, multispin_dev.h): the same bits.
//
// k9_measure: per-sample integers of every plane in one launch: unsatisfied bonds, set spins, and with two replicas the differing spins
// and the differing bonds of the pair.  A lane adds its sites' one-bit words into bit-sliced vertical counters (8 planes: at most
// 192 additions per lane), expands them per bit into LDS counters of the workgroup, and the workgroup adds those with 64-bit
// vector atomics.
//
// The handle and what builds the kernels' parameters from it live in multispin_host.h, shared with multispin_pt.hip (tempering:
// the swap plan and the masked exchange), which takes its measurements through msc_enqueue_measure below.
#include <cmath>
#include <new>
#include <vector>

#include "multispin_host.h"

namespace {

constexpr int kSmallLanes = 1024;
constexpr int kSmallSites = 8192;   // 64 KiB of spins
constexpr int kSmallBlocks = 1024;  // octets of a plane the small route stages uniforms for
constexpr int kAhead = 4;           // half-sweeps of Philox blocks computed ahead
constexpr int kMeasureSites = 64;   // sites per lane of k9_measure: 3 additions each into 8-plane counters

__device__ __forceinline__ uint32_t msc_shfl(uint32_t v, int src) {
    return (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)v);
}

__global__ __launch_bounds__(256) void k9_sweep(MscParams p, uint32_t hs, int colour) {
    __shared__ uint64_t tab[13];
    const int plane = blockIdx.z;
    const int ta = plane / p.W, w = plane - ta * p.W;
    if (threadIdx.x < 13) tab[threadIdx.x] = p.tab[13 * (ta / p.A) + threadIdx.x];
    __syncthreads();
    const uint32_t k0 = p.key[2 * ta], k1 = p.key[2 * ta + 1];
    const MscGeo g = p.g;
    uint64_t* s = p.s + (long long)plane * g.nsites;
    const uint64_t* jr = p.j + (long long)w * g.nsites;
    const uint64_t* jd = p.j + (long long)(p.W + w) * g.nsites;
    const uint64_t* jl = p.j + (long long)(2 * p.W + w) * g.nsites;
    const int lane = threadIdx.x & 63;
    const int b0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    // this lane's octet: its coordinates and its block, for the eight lanes that update it
    const int mine = b0 + lane;
    const bool live = mine < g.nblk;
    const int rho = live ? mine / g.noct : 0;
    const int myq = live ? mine - rho * g.noct : 0;
    const int myz = rho / g.rows, myr = rho - myz * g.rows;
    const u32x4 hv = tsu_philox((uint32_t)myq, (uint32_t)rho, hs, TSU_TAG_ISING_HI, k0, k1);
    const int m = lane & 7;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int src = 8 * i + (lane >> 3);
        const uint32_t w0 = msc_shfl(hv.x, src), w1 = msc_shfl(hv.y, src), w2 = msc_shfl(hv.z, src), w3 = msc_shfl(hv.w, src);
        const int z = (int)msc_shfl((uint32_t)myz, src), r = (int)msc_shfl((uint32_t)myr, src), q = (int)msc_shfl((uint32_t)myq, src);
        const int c = 16 * q + 2 * m + ((z + r + colour) & 1);
        if (b0 + src < g.nblk && c < g.cols)
            s[(z * g.rows + r) * g.cols + c] = msc_site(s, jr, jd, jl, g, z, r, c, q, m, msc_hi16(w0, w1, w2, w3, m), tab, hs, k0, k1);
    }
}

__global__ __launch_bounds__(kSmallLanes) void k9_small(MscParams p, int n_sweeps, uint32_t sweep0) {
    extern __shared__ __align__(16) uint64_t lds[];
    const MscGeo g = p.g;
    uint64_t* s = lds;                                           // nsites words
    uint64_t* tab = lds + ((g.nsites + 1) & ~1);                 // 13 (+ 1: the blocks stay 16-byte aligned)
    uint32_t* uni = reinterpret_cast<uint32_t*>(tab + 14);       // kAhead * nblk blocks of 4 words
    uint32_t* blk = uni + 4 * kAhead * g.nblk;                   // octet -> z << 16 | r
    const int plane = blockIdx.x, tid = threadIdx.x;
    const int ta = plane / p.W, w = plane - ta * p.W;
    const uint32_t k0 = p.key[2 * ta], k1 = p.key[2 * ta + 1];
    uint64_t* gs = p.s + (long long)plane * g.nsites;
    const uint64_t* jr = p.j + (long long)w * g.nsites;
    const uint64_t* jd = p.j + (long long)(p.W + w) * g.nsites;
    const uint64_t* jl = p.j + (long long)(2 * p.W + w) * g.nsites;
    for (int i = tid; i < g.nsites; i += kSmallLanes) s[i] = gs[i];
    if (tid < 13) tab[tid] = p.tab[13 * (ta / p.A) + tid];
    for (int b = tid; b < g.nblk; b += kSmallLanes) {
        const int rho = b / g.noct, z = rho / g.rows;
        blk[b] = ((uint32_t)z << 16) | (uint32_t)(rho - z * g.rows);
    }
    __syncthreads();
    const int total = 2 * n_sweeps;
    for (int h0 = 0; h0 < total; h0 += kAhead) {
        const int nh = min(kAhead, total - h0);
        const uint32_t hs0 = 2u * sweep0 + (uint32_t)h0;
        for (int item = tid; item < nh * g.nblk; item += kSmallLanes) {
            const int h = item / g.nblk, b = item - h * g.nblk;
            const int z = (int)(blk[b] >> 16), r = (int)(blk[b] & 0xFFFFu), rho = z * g.rows + r;
            const u32x4 hv = tsu_philox((uint32_t)(b - rho * g.noct), (uint32_t)rho, hs0 + (uint32_t)h, TSU_TAG_ISING_HI, k0, k1);
            *reinterpret_cast<uint4*>(uni + 4 * item) = make_uint4(hv.x, hv.y, hv.z, hv.w);
        }
        __syncthreads();
        for (int h = 0; h < nh; ++h) {
            const int colour = h & 1;  // h0 is even
            for (int t = tid; t < 8 * g.nblk; t += kSmallLanes) {
                const int b = t >> 3, m = t & 7;
                const int z = (int)(blk[b] >> 16), r = (int)(blk[b] & 0xFFFFu), rho = z * g.rows + r;
                const int q = b - rho * g.noct;
                const int c = 16 * q + 2 * m + ((z + r + colour) & 1);
                if (c < g.cols) {
                    const uint32_t word = uni[4 * (h * g.nblk + b) + (m >> 1)];
                    const uint32_t hi = ((word >> (16 * (m & 1))) & 0xFFFFu) ^ 0x8000u;
                    s[rho * g.cols + c] = msc_site(s, jr, jd, jl, g, z, r, c, q, m, hi, tab, hs0 + (uint32_t)h, k0, k1);
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < g.nsites; i += kSmallLanes) gs[i] = s[i];
}

// every sample of plane (t, a) starts from k8_randomize's bits for the key of (t, a), replica 0
__global__ __launch_bounds__(256) void k9_randomize(MscParams p) {
    const MscGeo g = p.g;
    const int plane = blockIdx.y, ta = plane / p.W;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.nsites) return;
    const int rho = i / g.cols, c = i - rho * g.cols, q = c >> 4;
    const u32x4 v = tsu_philox((uint32_t)(q >> 3), (uint32_t)rho, 0u, TSU_TAG_INIT, p.key[2 * ta], p.key[2 * ta + 1]);
    const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
    const uint32_t bits = (wv[(q & 7) >> 1] >> (16 * (q & 1))) & 0xFFFFu;
    p.s[(long long)plane * g.nsites + i] = ((bits >> (c & 15)) & 1u) ? ~0ull : 0ull;
}

// out: [unsat: nT A W 64][up: nT A W 64][qx: nT W 64][lx: nT W 64] counts.  Grid (ceil(nsites / (256 kMeasureSites)), nT W).
template <int A>
__global__ __launch_bounds__(256) void k9_measure(MscParams p, unsigned long long* __restrict__ out) {
    constexpr int Q = A == 2 ? 6 : 2;  // unsat a, up a, (unsat b, up b, spins differ, bonds differ)
    __shared__ uint32_t acc[Q][64];
    const MscGeo g = p.g;
    const int t = blockIdx.y / p.W, w = blockIdx.y - t * p.W;
    const int tid = threadIdx.x;
    for (int k = tid; k < Q * 64; k += 256) (&acc[0][0])[k] = 0;
    __syncthreads();
    const uint64_t* sa = p.s + (long long)((t * A) * p.W + w) * g.nsites;
    const uint64_t* sb = p.s + (long long)((t * A + A - 1) * p.W + w) * g.nsites;
    const uint64_t* jr = p.j + (long long)w * g.nsites;
    const uint64_t* jd = p.j + (long long)(p.W + w) * g.nsites;
    const uint64_t* jl = p.j + (long long)(2 * p.W + w) * g.nsites;
    MscCount<8> cnt[Q];
#pragma unroll
    for (int k = 0; k < Q; ++k) cnt[k].clear();
    bool any = false;
    for (int k = 0; k < kMeasureSites; ++k) {
        const long long i64 = ((long long)blockIdx.x * kMeasureSites + k) * 256 + tid;
        if (i64 >= g.nsites) break;
        any = true;
        const int i = (int)i64;
        const int rho = i / g.cols, c = i - rho * g.cols, z = rho / g.rows, r = rho - z * g.rows;
        // the bonds of the energy: right, down, layer, those an open axis lacks dropped
        const int nb[3] = {rho * g.cols + (c + 1 < g.cols ? c + 1 : 0), (z * g.rows + (r + 1 < g.rows ? r + 1 : 0)) * g.cols + c,
                           ((z + 1 < g.depth ? z + 1 : 0) * g.rows + r) * g.cols + c};
        const bool has[3] = {c + 1 < g.cols || g.pc != 0, r + 1 < g.rows || g.pr != 0, z + 1 < g.depth || g.pz != 0};
        const uint64_t* jj[3] = {jr, jd, jl};
        const uint64_t a = sa[i];
        cnt[1].add(a);
        uint64_t b = 0;
        if constexpr (A == 2) {
            b = sb[i];
            cnt[3].add(b);
            cnt[4].add(a ^ b);
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            if (!has[d]) continue;
            const uint64_t da = a ^ sa[nb[d]];
            cnt[0].add(da ^ jj[d][i]);  // s_i s_j J = -1
            if constexpr (A == 2) {
                const uint64_t db = b ^ sb[nb[d]];
                cnt[2].add(db ^ jj[d][i]);
                cnt[5].add(da ^ db);
            }
        }
    }
    if (any) {
        const int lane = tid & 63;
        for (int k = 0; k < 64; ++k) {
            const int bit = (k + lane) & 63;
#pragma unroll
            for (int qn = 0; qn < Q; ++qn) {
                const uint32_t v = cnt[qn].value(bit);
                if (v) atomicAdd(&acc[qn][bit], v);
            }
        }
    }
    __syncthreads();
    const long long col = 64ll * p.W;  // columns of one (t, a) row
    const long long n1 = (long long)(gridDim.y / p.W) * A * col;  // entries of unsat (and of up)
    const long long nq = (long long)(gridDim.y / p.W) * col;
    for (int k = tid; k < Q * 64; k += 256) {
        const int qn = k >> 6, bit = k & 63;
        const uint32_t v = acc[qn][bit];
        if (!v) continue;
        long long at;
        if (qn < 4) at = (qn & 1) * n1 + ((long long)(t * A + (qn >> 1)) * p.W + w) * 64 + bit;
        else at = 2 * n1 + (qn - 4) * nq + ((long long)t * p.W + w) * 64 + bit;
        atomicAdd(out + at, (unsigned long long)v);
    }
}

size_t msc_small_lds(const MscGeo& g) {
    return (size_t)((g.nsites + 1) & ~1) * 8 + 14 * 8 + (size_t)kAhead * g.nblk * 16 + (size_t)g.nblk * 4;
}

bool msc_fits_small(const MscGeo& g) { return g.nsites <= kSmallSites && g.nblk <= kSmallBlocks; }

}  // namespace

hipError_t msc_enqueue_sweeps(tsu_msc* h, int n_sweeps, uint32_t sweep0, unsigned long long* launches) {
    if (n_sweeps <= 0) return hipSuccess;
    const MscParams p = msc_params(h);
    const unsigned planes = (unsigned)msc_planes(h);
    if (h->route == TSU_MSC_ROUTE_SMALL) {
        k9_small<<<planes, kSmallLanes, msc_small_lds(h->g), h->ctx->stream>>>(p, n_sweeps, sweep0);
        *launches += 1;
    } else {
        const dim3 grid((unsigned)((h->g.nblk + 255) / 256), 1, planes);
        for (int s = 0; s < n_sweeps; ++s)
            for (int colour = 0; colour < 2; ++colour) {
                k9_sweep<<<grid, 256, 0, h->ctx->stream>>>(p, 2u * (sweep0 + (uint32_t)s) + (uint32_t)colour, colour);
                *launches += 1;
            }
    }
    return hipGetLastError();
}

hipError_t msc_enqueue_measure(tsu_msc* h, unsigned long long* row) {
    const dim3 grid((unsigned)((h->g.nsites + 256 * kMeasureSites - 1) / (256 * kMeasureSites)), (unsigned)(h->nT * h->W), 1);
    if (h->A == 2) k9_measure<2><<<grid, 256, 0, h->ctx->stream>>>(msc_params(h), row);
    else k9_measure<1><<<grid, 256, 0, h->ctx->stream>>>(msc_params(h), row);
    return hipGetLastError();
}

extern "C" {

int tsu_msc_thresholds(double T, uint64_t table[13]) {
    if (!table || !(T > 0.0) || !std::isfinite(T)) return TSU_E_INVALID;
    for (int f = -6; f <= 6; ++f) {
        const double x = (2.0 * (double)f) / T;
        const double prob = x > 20.0 ? 1.0 : (x < -20.0 ? 0.0 : 1.0 / (1.0 + exp(-x)));
        table[f + 6] = (uint64_t)floor(prob * 4294967296.0 + 0.5);
    }
    return TSU_OK;
}

int tsu_msc_create(tsu_ctx* ctx, int depth, int rows, int cols, int periodic_mask, int n_temps, int replicas, int n_samples, int route,
                   tsu_msc** out) {
    TSU_ENTER(ctx);
    if (!ctx || !out) return TSU_E_INVALID;
    *out = nullptr;
    TSU_REQUIRE(ctx, depth >= 1 && rows >= 1 && cols >= 1, "msc: depth/rows/cols must be positive");
    TSU_REQUIRE(ctx, (periodic_mask & ~7) == 0, "msc: periodic_mask must be a combination of TSU_PERIODIC_Z / _R / _C, got %d", periodic_mask);
    TSU_REQUIRE(ctx, n_temps >= 1 && n_samples >= 1, "msc: n_temps and n_samples must be positive");
    TSU_REQUIRE(ctx, replicas == 1 || replicas == 2, "msc: replicas must be 1 or 2, got %d", replicas);
    TSU_REQUIRE(ctx, route >= TSU_MSC_ROUTE_AUTO && route <= TSU_MSC_ROUTE_HBM, "msc: bad route %d", route);
    TSU_REQUIRE(ctx, (long long)depth * rows * cols <= (1ll << 30), "msc: lattice too large for 32-bit site indices");
    const int len[3] = {depth, rows, cols};
    const char* axis[3] = {"depth", "rows", "cols"};
    for (int a = 0; a < 3; ++a)
        if (((periodic_mask >> a) & 1) && ((len[a] & 1) || len[a] < 4))
            return tsu_fail(ctx, TSU_E_UNSUPPORTED, "msc: a periodic axis needs an even length >= 4 (%s = %d)", axis[a], len[a]);
    const int W = (n_samples + 63) / 64;
    const long long planes = (long long)n_temps * replicas * W;
    TSU_REQUIRE(ctx, planes <= 65535, "msc: n_temps x replicas x ceil(n_samples / 64) = %lld planes exceed 65535", planes);
    MscGeo g = {};
    g.depth = depth;
    g.rows = rows;
    g.cols = cols;
    g.pz = (periodic_mask >> 0) & 1;
    g.pr = (periodic_mask >> 1) & 1;
    g.pc = (periodic_mask >> 2) & 1;
    g.noct = (cols + 15) / 16;
    g.nsites = depth * rows * cols;
    TSU_REQUIRE(ctx, (long long)depth * rows * g.noct < (1ll << 31), "msc: too many octets");
    g.nblk = depth * rows * g.noct;
    if (route == TSU_MSC_ROUTE_SMALL && !msc_fits_small(g))
        return tsu_fail(ctx, TSU_E_UNSUPPORTED, "msc: the small route takes planes of at most %d sites and %d octets (%d sites, %d octets)",
                        kSmallSites, kSmallBlocks, g.nsites, g.nblk);
    tsu_msc* h = new (std::nothrow) tsu_msc();
    if (!h) return tsu_fail(ctx, TSU_E_NOMEM, "msc: host allocation failed");
    h->ctx = ctx;
    h->g = g;
    h->nT = n_temps;
    h->A = replicas;
    h->S = n_samples;
    h->W = W;
    h->route = route == TSU_MSC_ROUTE_AUTO ? (msc_fits_small(g) ? TSU_MSC_ROUTE_SMALL : TSU_MSC_ROUTE_HBM) : route;
    const size_t sbytes = (size_t)planes * g.nsites * 8, jbytes = (size_t)3 * W * g.nsites * 8;
    const size_t obytes = ((size_t)2 * n_temps * replicas + 2 * n_temps) * W * 64 * 8;
    hipError_t e = hipMalloc((void**)&h->d_s, sbytes);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_s, 0, sbytes, ctx->stream);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_j, jbytes);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_j, 0, jbytes, ctx->stream);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_tab, (size_t)n_temps * 13 * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_key, (size_t)n_temps * replicas * 2 * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_out, obytes);
    if (e == hipSuccess && h->route == TSU_MSC_ROUTE_SMALL)
        e = tsu_func_allow_lds(ctx, reinterpret_cast<const void*>(k9_small), (int)msc_small_lds(g));
    if (e != hipSuccess) {
        const int rc = tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "msc_create: %s (%zu bytes of planes)",
                                hipGetErrorString(e), sbytes);
        tsu_msc_destroy(h);
        return rc;
    }
    *out = h;
    return TSU_OK;
}

int tsu_msc_destroy(tsu_msc* h) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_OK;
    (void)hipStreamSynchronize(h->ctx->stream);
    msc_pt_free(h);
    msc_corr_free(h);
    msc_quench_free(h);
    if (h->d_s) (void)hipFree(h->d_s);
    if (h->d_j) (void)hipFree(h->d_j);
    if (h->d_tab) (void)hipFree(h->d_tab);
    if (h->d_key) (void)hipFree(h->d_key);
    if (h->d_out) (void)hipFree(h->d_out);
    delete h;
    return TSU_OK;
}

int tsu_msc_route(tsu_msc* h, int* route) {
    if (!h || !route) return TSU_E_INVALID;
    *route = h->route;
    return TSU_OK;
}

int tsu_msc_set_couplings(tsu_msc* h, const uint64_t* J_right, const uint64_t* J_down, const uint64_t* J_layer) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    TSU_REQUIRE(ctx, J_right && J_down && (J_layer || h->g.depth == 1), "msc_set_couplings: J_right, J_down and J_layer are required");
    const size_t n = (size_t)h->W * h->g.nsites;
    const uint64_t* src[3] = {J_right, J_down, J_layer};
    for (int k = 0; k < 3; ++k) {
        if (src[k]) TSU_HIP_TRY(ctx, hipMemcpyAsync(h->d_j + k * n, src[k], n * 8, hipMemcpyHostToDevice, ctx->stream));
        else TSU_HIP_TRY(ctx, hipMemsetAsync(h->d_j + k * n, 0, n * 8, ctx->stream));
    }
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int tsu_msc_set_planes(tsu_msc* h, const uint64_t* planes) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    TSU_REQUIRE(ctx, planes, "msc_set_planes: NULL input");
    TSU_HIP_TRY(ctx, hipMemcpyAsync(h->d_s, planes, msc_planes(h) * h->g.nsites * 8, hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int tsu_msc_get_planes(tsu_msc* h, uint64_t* planes) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    TSU_REQUIRE(ctx, planes, "msc_get_planes: NULL output");
    TSU_HIP_TRY(ctx, hipMemcpyAsync(planes, h->d_s, msc_planes(h) * h->g.nsites * 8, hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int tsu_msc_set_seeds(tsu_msc* h, const uint64_t* seeds) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    TSU_REQUIRE(ctx, seeds, "msc_set_seeds: NULL input");
    const int n = h->nT * h->A;
    std::vector<uint32_t> key(2 * (size_t)n);
    for (int i = 0; i < n; ++i) {
        key[2 * i] = (uint32_t)seeds[i];
        key[2 * i + 1] = (uint32_t)(seeds[i] >> 32);
    }
    TSU_HIP_TRY(ctx, hipMemcpyAsync(h->d_key, key.data(), key.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    h->have_seeds = 1;
    return TSU_OK;
}

int tsu_msc_randomize(tsu_msc* h) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    TSU_REQUIRE(ctx, h->have_seeds, "msc_randomize: call tsu_msc_set_seeds first");
    k9_randomize<<<dim3((unsigned)((h->g.nsites + 255) / 256), (unsigned)msc_planes(h), 1), 256, 0, ctx->stream>>>(msc_params(h));
    TSU_HIP_TRY(ctx, hipGetLastError());
    return TSU_OK;
}

int tsu_msc_fill(tsu_msc* h, int8_t value) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    TSU_REQUIRE(ctx, value == 1 || value == -1, "msc_fill: value must be +1 or -1");
    TSU_HIP_TRY(ctx, hipMemsetAsync(h->d_s, value == 1 ? 0xFF : 0x00, msc_planes(h) * h->g.nsites * 8, ctx->stream));
    return TSU_OK;
}

int tsu_msc_set_temperatures(tsu_msc* h, const double* T) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    TSU_REQUIRE(ctx, T, "msc_set_temperatures: NULL input");
    std::vector<uint64_t> tab(13 * (size_t)h->nT);
    for (int t = 0; t < h->nT; ++t) TSU_REQUIRE(ctx, tsu_msc_thresholds(T[t], tab.data() + 13 * t) == TSU_OK, "Temperature must be positive");
    TSU_HIP_TRY(ctx, hipMemcpyAsync(h->d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    h->have_T = 1;
    return TSU_OK;
}

int tsu_msc_sweep(tsu_msc* h, int n_sweeps, uint32_t sweep0) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    TSU_REQUIRE(ctx, h->have_T && h->have_seeds, "msc_sweep: call tsu_msc_set_temperatures and tsu_msc_set_seeds first");
    TSU_REQUIRE(ctx, n_sweeps >= 0, "msc_sweep: n_sweeps must be >= 0");
    TSU_REQUIRE(ctx, (uint64_t)sweep0 + (uint64_t)n_sweeps <= (1ull << 31), "msc_sweep: sweep counter overflow");
    TSU_HIP_TRY(ctx, msc_enqueue_sweeps(h, n_sweeps, sweep0, &h->launches));
    return TSU_OK;
}

int tsu_msc_measure(tsu_msc* h, int64_t* unsat, int64_t* sum, int64_t* q, int64_t* q_link) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    TSU_REQUIRE(ctx, unsat && sum, "msc_measure: NULL output");
    const size_t col = (size_t)h->W * 64, n1 = (size_t)h->nT * h->A * col, nq = (size_t)h->nT * col;
    const size_t total = 2 * n1 + 2 * nq;
    TSU_HIP_TRY(ctx, hipMemsetAsync(h->d_out, 0, total * 8, ctx->stream));
    TSU_HIP_TRY(ctx, msc_enqueue_measure(h, h->d_out));
    std::vector<unsigned long long> host(total);
    TSU_HIP_TRY(ctx, hipMemcpyAsync(host.data(), h->d_out, total * 8, hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const long long N = h->g.nsites, nb = msc_bonds(h->g);
    for (size_t i = 0; i < n1; ++i) {
        unsat[i] = (int64_t)host[i];
        sum[i] = 2 * (int64_t)host[n1 + i] - N;
    }
    if (h->A == 2)
        for (size_t i = 0; i < nq; ++i) {
            if (q) q[i] = N - 2 * (int64_t)host[2 * n1 + i];
            if (q_link) q_link[i] = nb - 2 * (int64_t)host[2 * n1 + nq + i];
        }
    return TSU_OK;
}

int tsu_msc_launch_count(tsu_msc* h, uint64_t* out) {
    if (!h || !out) return TSU_E_INVALID;
    *out = h->launches;
    return TSU_OK;
}

}  // extern "C"

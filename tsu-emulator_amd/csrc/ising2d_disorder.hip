// ising2d_disorder.hip -- K7: heat-bath sweeps of a 2-D lattice with per-bond couplings and per-site fields (gfx950).
//
// Quenched disorder on the lattice handle: J_right[r][c] (bond (r, c)-(r, c+1), wrapping to column 0 on a periodic lattice),
// J_down[r][c] (bond (r, c)-(r+1, c), wrapping to row 0) and h[r][c], fp32, row-major.  Device copies use the spin buffer's
// pitch (in elements), pad columns 0.  Decision rule (the bit-exact contract):
//   f   = (((J_down[r-1][c] s_up + J_down[r][c] s_down) + J_right[r][c-1] s_left) + J_right[r][c] s_right) + h[r][c] in float64,
//         a missing neighbour of an open lattice skipped (no +0.0);  x = 2 f / T;  p = sigmoid(x) clamped at +-20;
//   thr = floor(p 2^32 + 1/2);  the site becomes +1 iff u < thr, u = K1's own 32-bit site uniform (same counters, same tags:
//         hi16 = half (m & 1) of Philox(c >> 4, r, hs, TAG_ISING_HI | replica << 8)[m >> 1] ^ 0x8000, m = (c >> 1) & 7; lo16
//         from TAG_ISING_LO, drawn only when hi16 ties with thr's top 16 bits).
// With the 25-entry table replaced by this per-site threshold, a constant dyadic (J, h) gives K1's spins bit for bit.
//
// k7_sweep: one launch per half-sweep, one lane per octet (16 consecutive columns of one row = 8 sites of the colour, the
// unit of one Philox block), 64 x 4 lanes per workgroup = one row per wave, so the column parity of the colour is uniform
// in a wave.  The lane screens its 8 sites in fp32 and only takes the float64 threshold of the contract where the fp32
// probability lies within a margin of the hi16 uniform (see screen() for the bound).  The spins are updated in place (a
// colour reads only the other colour), 16-byte masked stores, pad bytes untouched.  Every whole lattice K1 takes runs here
// (one-row and one-column lattices included); slabs are refused.
//
// Bytes: per half-sweep the launch reads every byte of the three disorder rows it touches (12 B per site: the lines hold both
// colours) and the spins (~3 B per site, up / down rows from L2), writes 1 B per site: ~28 B per site and sweep against the
// 2 B + 12 B / s of a tile-resident design.
//
// k7_energy + k7_energy_final: E = -sum_bonds J s s' - sum h s in float64, per-workgroup partials then one workgroup
// summing them in a fixed order (the same bits on every call).  k7_overlap: q = sum s^a s^b (integer, vector atomics).
#include <cmath>

#include "ising2d.h"

namespace {

constexpr int kEnergyBlocks = 1024;  // fixed partial count: the summation order depends on the shape only

struct K7Params {
    int8_t* s;           // owned row 0 of the current spin buffer
    const float* jr;     // J_right, J_down, h: row pitch = `pitch` elements
    const float* jd;
    const float* h;
    long long pitch;
    int rows, cols, periodic;
    float c32;           // fl32(2 / T): the screen's scale
    double T;
    uint32_t k0, k1, hs, tag_hi, tag_lo;
};

__device__ __forceinline__ int sbyte(const uint4& v, int i) {
    const uint32_t w = i < 4 ? v.x : (i < 8 ? v.y : (i < 12 ? v.z : v.w));
    return (int)(int8_t)((w >> (8 * (i & 3))) & 0xFFu);
}

__device__ __forceinline__ float fat(const float4* a, int i) {
    const float4 v = a[i >> 2];
    const int k = i & 3;
    return k == 0 ? v.x : (k == 1 ? v.y : (k == 2 ? v.z : v.w));
}

__device__ __forceinline__ void load16f(const float* p, float4* a) {
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = reinterpret_cast<const float4*>(p)[k];
}

// Threshold of the contract in float64 (sigmoid clamped at +-20 as tsu_ising2d_thresholds / gibbs.py:73-77)
__device__ __forceinline__ uint64_t exact_thr(double f, double T) {
    const double x = (2.0 * f) / T;
    const double p = x > 20.0 ? 1.0 : (x < -20.0 ? 0.0 : 1.0 / (1.0 + exp(-x)));
    return (uint64_t)floor(p * 4294967296.0 + 0.5);
}

// fp32 screen.  Returns +1 (u < thr for every low half), -1 (u >= thr for every low half) or 0 (decide exactly).
// t = p32 2^16 is compared with the hi16 uniform: u in [hi 2^16, hi 2^16 + 65535] is below thr for sure when
// t - dt >= hi + 1 and not below it when t + dt <= hi, dt a bound of |t - thr / 2^16|.  With u = 2^-24, S = the sum of the
// |terms| and A = 2 S / T:  four fp32 additions err by <= 4 u S; times fl(2 / T) adds 2 u |x|: |dx| <= 7 u A.  __expf
// (v_exp_f32 on x log2 e) errs by <= (|x| + 2) u relative, so e = exp(-x) by <= (9 A + 4) u relative (|x| <= A);
// p = rcp(1 + e) moves by p (1 - p) <= 1/4 of that plus 3 u p of its own rounding: |dp| <= (2.25 A + 4) u + 3 u.  The
// +-20 clamp of the exact p adds 2.1e-9 = 2^-28.9, and the rounding of thr half a unit of 2^-32.  In units of 2^-16:
// dt <= ((2.25 A + 7) + 2^-4.9) / 256 + 2^-17 < (A + 4) / 64 = the margin below (a factor >= 1.7 to spare).  Non-finite
// A or t (huge disorder, tiny T) fail both comparisons and go to the exact branch.
__device__ __forceinline__ int screen(float f32, float a32, float c32, uint32_t hi) {
    const float x = f32 * c32;
    const float A = a32 * fabsf(c32);
    const float t = __builtin_amdgcn_rcpf(1.0f + __expf(-x)) * 65536.0f;
    const float m = (A + 4.0f) * (1.0f / 64.0f);
    const float h = (float)hi;
    if (t >= h + 1.0f + m) return 1;
    if (t <= h - m) return -1;
    return 0;
}

// one octet of the colour whose sites sit at chunk positions PAR, PAR + 2, ..
template <int PAR>
__device__ __forceinline__ void k7_octet(const K7Params& p, int r, int q) {
    const long long row = (long long)r * p.pitch;
    const int c0 = 16 * q;
    const bool has_up = r > 0 || p.periodic, has_dn = r + 1 < p.rows || p.periodic;
    const long long rowu = (long long)(r > 0 ? r - 1 : p.rows - 1) * p.pitch;
    const long long rowd = (long long)(r + 1 < p.rows ? r + 1 : 0) * p.pitch;
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    const uint4 C = *reinterpret_cast<const uint4*>(p.s + row + c0);
    const uint4 U = has_up ? *reinterpret_cast<const uint4*>(p.s + rowu + c0) : zero4;
    const uint4 D = has_dn ? *reinterpret_cast<const uint4*>(p.s + rowd + c0) : zero4;
    float4 jr[4], jd[4], ju[4], hh[4];
    load16f(p.jr + row + c0, jr);
    load16f(p.jd + row + c0, jd);
    load16f(p.h + row + c0, hh);
    if (has_up) load16f(p.jd + rowu + c0, ju);
    else
        for (int k = 0; k < 4; ++k) ju[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    // column c0 - 1 (left of position 0), column c0 + 16 (right of position 15), column 0 (right of the last column, periodic)
    const bool has_prev = q > 0 || p.periodic;
    const int cprev = q > 0 ? c0 - 1 : p.cols - 1;
    const int s_prev = has_prev ? (int)p.s[row + cprev] : 0;
    const float j_prev = has_prev ? p.jr[row + cprev] : 0.0f;
    const int s_next = (c0 + 16 < p.cols) ? (int)p.s[row + c0 + 16] : 0;
    const int s_first = p.periodic ? (int)p.s[row] : 0;

    const u32x4 w = tsu_philox((uint32_t)q, (uint32_t)r, p.hs, p.tag_hi, p.k0, p.k1);
    const uint32_t wv[4] = {w.x, w.y, w.z, w.w};
    bool have_lo = false;
    uint32_t lv[4] = {0, 0, 0, 0};
    uint32_t out[4] = {C.x, C.y, C.z, C.w};
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int i = 2 * m + PAR, c = c0 + i;
        if (c >= p.cols) break;
        const bool has_left = i > 0 || has_prev, has_right = c + 1 < p.cols || p.periodic;
        const int su = sbyte(U, i), sd = sbyte(D, i);
        const int sl = i > 0 ? sbyte(C, i - 1) : s_prev;
        const int sr = c + 1 < p.cols ? (i < 15 ? sbyte(C, i + 1) : s_next) : s_first;
        const float Ju = has_up ? fat(ju, i) : 0.0f, Jd = has_dn ? fat(jd, i) : 0.0f;
        const float Jl = has_left ? (i > 0 ? fat(jr, i - 1) : j_prev) : 0.0f;
        const float Jr = has_right ? fat(jr, i) : 0.0f;
        const float hf = fat(hh, i);
        // missing neighbours carry J = 0 here: exact in fp32, and the screen only needs a bound
        const float f32 = (((Ju * (float)su + Jd * (float)sd) + Jl * (float)sl) + Jr * (float)sr) + hf;
        const float a32 = fabsf(Ju) + fabsf(Jd) + fabsf(Jl) + fabsf(Jr) + fabsf(hf);
        const uint32_t hi = ((wv[m >> 1] >> (16 * (m & 1))) & 0xFFFFu) ^ 0x8000u;
        int dec = screen(f32, a32, p.c32, hi);
        if (dec == 0) {
            // the contract's sum: neighbours in the order up, down, left, right, a missing one skipped, then h
            double f = 0.0;
            bool any = false;
            if (has_up) { f = (double)Ju * su; any = true; }
            if (has_dn) { f = any ? f + (double)Jd * sd : (double)Jd * sd; any = true; }
            if (has_left) { f = any ? f + (double)Jl * sl : (double)Jl * sl; any = true; }
            if (has_right) { f = any ? f + (double)Jr * sr : (double)Jr * sr; any = true; }
            f = any ? f + (double)hf : (double)hf;
            const uint64_t thr = exact_thr(f, p.T);
            const uint32_t thi = (uint32_t)(thr >> 16);
            bool accept = hi < thi;
            if (hi == thi) {  // tie on the top 16 bits: the low half, as K1 draws it
                if (!have_lo) {
                    const u32x4 l = tsu_philox((uint32_t)q, (uint32_t)r, p.hs, p.tag_lo, p.k0, p.k1);
                    lv[0] = l.x; lv[1] = l.y; lv[2] = l.z; lv[3] = l.w;
                    have_lo = true;
                }
                const uint32_t lo = (lv[m >> 1] >> (16 * (m & 1))) & 0xFFFFu;
                accept = (((uint64_t)hi << 16) | lo) < thr;
            }
            dec = accept ? 1 : -1;
        }
        const uint32_t b = dec > 0 ? 0x01u : 0xFFu;
        const int sh = 8 * (i & 3);
        out[i >> 2] = (out[i >> 2] & ~(0xFFu << sh)) | (b << sh);
    }
    *reinterpret_cast<uint4*>(p.s + row + c0) = make_uint4(out[0], out[1], out[2], out[3]);
}

// grid (ceil(nchunks / 64), ceil(rows / 4)), 64 x 4 lanes: lane = octet q of row r
__global__ __launch_bounds__(256) void k7_sweep(K7Params p, int colour) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    const int r = blockIdx.y * 4 + threadIdx.y;
    if (r >= p.rows || 16 * q >= p.cols) return;
    if (((r + colour) & 1) == 0) k7_octet<0>(p, r, q);
    else k7_octet<1>(p, r, q);
}

// E partials: lane = chunk (r, q), grid-stride in a fixed order, fixed shuffle tree, one partial per workgroup
__global__ __launch_bounds__(256) void k7_energy(K7Params p, double* __restrict__ part) {
    const int nchunks = (p.cols + 15) >> 4;
    const long long total = (long long)p.rows * nchunks;
    double e = 0.0;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const int r = (int)(t / nchunks), q = (int)(t - (long long)r * nchunks);
        const long long row = (long long)r * p.pitch;
        const bool has_dn = r + 1 < p.rows || p.periodic;
        const long long rowd = (long long)(r + 1 < p.rows ? r + 1 : 0) * p.pitch;
        for (int i = 0; i < 16; ++i) {
            const int c = 16 * q + i;
            if (c >= p.cols) break;
            const int s = p.s[row + c];
            double l = (double)p.h[row + c];
            if (c + 1 < p.cols || p.periodic) l += (double)p.jr[row + c] * p.s[row + (c + 1 < p.cols ? c + 1 : 0)];
            if (has_dn) l += (double)p.jd[row + c] * p.s[rowd + c];
            e += s * l;
        }
    }
    for (int off = 32; off > 0; off >>= 1) e += __shfl_down(e, off, 64);
    __shared__ double wpart[4];
    if ((threadIdx.x & 63) == 0) wpart[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (wpart[0] + wpart[1]) + (wpart[2] + wpart[3]);
}

// one workgroup: out[0] = -(sum of the n partials), in a fixed order
__global__ __launch_bounds__(256) void k7_energy_final(const double* __restrict__ part, int n, double* __restrict__ out) {
    double e = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) e += part[i];
    for (int off = 32; off > 0; off >>= 1) e += __shfl_down(e, off, 64);
    __shared__ double wpart[4];
    if ((threadIdx.x & 63) == 0) wpart[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = -((wpart[0] + wpart[1]) + (wpart[2] + wpart[3]));
}

// q = sum over sites of s^a s^b (columns < cols only), one 64-bit vector atomic per workgroup
__global__ __launch_bounds__(256) void k7_overlap(const int8_t* __restrict__ a, const int8_t* __restrict__ b, long long pitch_a,
                                                  long long pitch_b, int rows, int cols, long long* __restrict__ acc) {
    const int nchunks = (cols + 15) >> 4;
    const long long total = (long long)rows * nchunks;
    long long sum = 0;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const int r = (int)(t / nchunks), q = (int)(t - (long long)r * nchunks);
        const uint4 va = *reinterpret_cast<const uint4*>(a + r * pitch_a + 16 * q);
        const uint4 vb = *reinterpret_cast<const uint4*>(b + r * pitch_b + 16 * q);
        int cs = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (16 * q + i < cols) cs += sbyte(va, i) * sbyte(vb, i);
        sum += cs;
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    __shared__ long long wpart[4];
    if ((threadIdx.x & 63) == 0) wpart[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0)
        atomicAdd(reinterpret_cast<unsigned long long*>(acc), (unsigned long long)(wpart[0] + wpart[1] + wpart[2] + wpart[3]));
}

bool whole_lattice(const tsu_ising2d* L) { return L->ghost == 0 && L->row0 == 0 && L->total_rows == L->rows; }

K7Params make_params(const tsu_ising2d* L) {
    K7Params p;
    const size_t plane = (size_t)L->rows * L->pitch;
    p.s = L->alloc[L->cur];
    p.jr = L->d_dis;
    p.jd = L->d_dis ? L->d_dis + plane : nullptr;
    p.h = L->d_dis ? L->d_dis + 2 * plane : nullptr;
    p.pitch = (long long)L->pitch;
    p.rows = L->rows;
    p.cols = L->cols;
    p.periodic = L->periodic;
    p.c32 = 0.0f;
    p.T = 0.0;
    p.k0 = p.k1 = p.hs = p.tag_hi = p.tag_lo = 0;
    return p;
}

unsigned blocks_for(const tsu_ising2d* L) {
    const long long work = (long long)L->rows * ((L->cols + 15) / 16);
    const long long b = (work + 255) / 256;
    return (unsigned)(b < kEnergyBlocks ? b : kEnergyBlocks);
}

}  // namespace

extern "C" {

int tsu_ising2d_set_disorder(tsu_ising2d* L, const float* J_right, const float* J_down, const float* h) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, J_right && J_down, "ising2d_set_disorder: J_right and J_down are required (h may be NULL)");
    if (!whole_lattice(L)) return tsu_fail(ctx, TSU_E_UNSUPPORTED, "ising2d_set_disorder: whole lattices only (not a slab)");
    const int rows = L->rows, cols = L->cols;
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            const size_t i = (size_t)r * cols + c;
            TSU_REQUIRE(ctx, std::isfinite(J_right[i]) && std::isfinite(J_down[i]) && (!h || std::isfinite(h[i])),
                        "ising2d_set_disorder: non-finite value at site (%d, %d)", r, c);
            TSU_REQUIRE(ctx, L->periodic || c + 1 < cols || J_right[i] == 0.0f,
                        "ising2d_set_disorder: open lattice: J_right[%d, %d] (last column) must be 0, got %g", r, c, (double)J_right[i]);
            TSU_REQUIRE(ctx, L->periodic || r + 1 < rows || J_down[i] == 0.0f,
                        "ising2d_set_disorder: open lattice: J_down[%d, %d] (last row) must be 0, got %g", r, c, (double)J_down[i]);
        }
    const size_t plane = (size_t)rows * L->pitch;
    if (!L->d_dis) {
        TSU_HIP_TRY(ctx, hipMalloc((void**)&L->d_dis, 3 * plane * sizeof(float)));
        TSU_HIP_TRY(ctx, hipMemsetAsync(L->d_dis, 0, 3 * plane * sizeof(float), ctx->stream));  // pad columns stay 0
    }
    const size_t dpitch = L->pitch * sizeof(float), w = (size_t)cols * sizeof(float);
    TSU_HIP_TRY(ctx, hipMemcpy2DAsync(L->d_dis, dpitch, J_right, w, w, (size_t)rows, hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipMemcpy2DAsync(L->d_dis + plane, dpitch, J_down, w, w, (size_t)rows, hipMemcpyHostToDevice, ctx->stream));
    if (h) TSU_HIP_TRY(ctx, hipMemcpy2DAsync(L->d_dis + 2 * plane, dpitch, h, w, w, (size_t)rows, hipMemcpyHostToDevice, ctx->stream));
    else TSU_HIP_TRY(ctx, hipMemsetAsync(L->d_dis + 2 * plane, 0, plane * sizeof(float), ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    L->have_disorder = 1;
    return TSU_OK;
}

int tsu_ising2d_clear_disorder(tsu_ising2d* L) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    L->have_disorder = 0;  // the buffers stay for the next set_disorder (freed with the handle)
    return TSU_OK;
}

int tsu_ising2d_disorder_sweep(tsu_ising2d* L, double T, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, L->have_disorder, "ising2d_disorder_sweep: call tsu_ising2d_set_disorder first");
    TSU_REQUIRE(ctx, T > 0.0 && std::isfinite(T), "Temperature must be positive");
    TSU_REQUIRE(ctx, n_sweeps >= 0, "ising2d_sweep: n_sweeps must be >= 0");
    TSU_REQUIRE(ctx, (uint64_t)sweep0 + (uint64_t)n_sweeps <= (1ull << 31), "ising2d_sweep: sweep counter overflow");
    if (n_sweeps == 0) return TSU_OK;
    if (L->timing) TSU_HIP_TRY(ctx, hipEventRecord(L->ev0, ctx->stream));
    K7Params p = make_params(L);
    ising2d_set_keys(p, seed, replica);
    p.T = T;
    p.c32 = (float)(2.0 / T);
    const int nchunks = (L->cols + 15) >> 4;
    const dim3 grid((unsigned)((nchunks + 63) / 64), (unsigned)((L->rows + 3) / 4), 1);
    for (int s = 0; s < n_sweeps; ++s)
        for (int colour = 0; colour < 2; ++colour) {
            p.hs = 2u * (sweep0 + (uint32_t)s) + (uint32_t)colour;
            k7_sweep<<<grid, dim3(64, 4, 1), 0, ctx->stream>>>(p, colour);
            L->dis_launches += 1;
        }
    TSU_HIP_TRY(ctx, hipGetLastError());
    if (L->timing) {
        TSU_HIP_TRY(ctx, hipEventRecord(L->ev1, ctx->stream));
        L->timed = 1;
    }
    return TSU_OK;
}

int tsu_ising2d_disorder_energy(tsu_ising2d* L, double* E) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, E, "ising2d_disorder_energy: NULL output");
    TSU_REQUIRE(ctx, L->have_disorder, "ising2d_disorder_energy: call tsu_ising2d_set_disorder first");
    const unsigned blocks = blocks_for(L);
    TSU_HIP_TRY(ctx, ising2d_grow(L->d_dis_part, L->dis_part_cap, (kEnergyBlocks + 1) * sizeof(double)));
    const K7Params p = make_params(L);
    k7_energy<<<blocks, 256, 0, ctx->stream>>>(p, L->d_dis_part);
    k7_energy_final<<<1, 256, 0, ctx->stream>>>(L->d_dis_part, (int)blocks, L->d_dis_part + kEnergyBlocks);
    TSU_HIP_TRY(ctx, hipGetLastError());
    double e = 0.0;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(&e, L->d_dis_part + kEnergyBlocks, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *E = e;
    return ising2d_check_err(L);
}

int tsu_ising2d_overlap(tsu_ising2d* A, tsu_ising2d* B, int64_t* q) {
    TSU_ENTER(A ? A->ctx : nullptr);
    if (!A || !B) return TSU_E_INVALID;
    tsu_ctx* ctx = A->ctx;
    TSU_REQUIRE(ctx, q, "ising2d_overlap: NULL output");
    TSU_REQUIRE(ctx, B->ctx == ctx, "ising2d_overlap: the two lattices belong to different contexts");
    TSU_REQUIRE(ctx, A->rows == B->rows && A->cols == B->cols && A->total_rows == B->total_rows,
                "ising2d_overlap: shapes differ (%d x %d against %d x %d)", A->rows, A->cols, B->rows, B->cols);
    TSU_REQUIRE(ctx, whole_lattice(A) && whole_lattice(B), "ising2d_overlap: whole lattices only (not slabs)");
    TSU_HIP_TRY(ctx, hipMemsetAsync(A->d_obs, 0, sizeof(int64_t), ctx->stream));
    k7_overlap<<<blocks_for(A), 256, 0, ctx->stream>>>(A->alloc[A->cur], B->alloc[B->cur], (long long)A->pitch, (long long)B->pitch,
                                                       A->rows, A->cols, (long long*)A->d_obs);
    TSU_HIP_TRY(ctx, hipGetLastError());
    int64_t h = 0;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(&h, A->d_obs, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *q = h;
    int rc = ising2d_check_err(A);
    return rc != TSU_OK ? rc : ising2d_check_err(B);
}

int tsu_ising2d_disorder_launch_count(tsu_ising2d* L, uint64_t* n) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L || !n) return TSU_E_INVALID;
    *n = L->dis_launches;
    return TSU_OK;
}

}  // extern "C"

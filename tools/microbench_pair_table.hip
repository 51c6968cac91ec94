// microbench_pair_table.hip -- what does the compare section of the K1 pair loop (csrc/ising2d_tiled.hip) cost when the 16-bit
// thresholds of a site pair come from a 25-dword LDS table instead of v_perm_b32 byte look-ups?
//   perm form  (compare_octet today): 4 v_perm pick the high / low threshold bytes by the byte counts, 4 v_perm interleave them
//              into the 16-bit fields of v_pk_sub_i16: 8 v_perm + 4 v_pk_sub_i16 per octet
//   table form: v_dot4_u32_u8(cnt, weights, 0) with byte weights (4, 20, 0, 0) / (0, 0, 4, 20) is the byte offset 4 c0 + 20 c1 of the
//              dword t16(c0) | t16(c1) << 16 in a table of 25 dwords: 4 v_dot4 + 4 ds_read_b32 + 4 v_pk_sub_i16 per octet
//   quad form:  the counts arrive scaled by 8 (up-flags stored as 8) and v_dot4_u32_u8(cnt8, weights, 0) with byte weights
//              (1, 5, 25, 125) is the byte offset 8 (c0 + 5 c1 + 25 c2 + 125 c3) of the four thresholds of a whole count dword in a
//              table of 625 x 8 bytes: 2 v_dot4 + 2 ds_read_b64 + 4 v_pk_sub_i16 per octet (profiles/k1_quad_table_microbench.txt)
// Timed kernels, one 1024-thread workgroup per CU (4 waves per SIMD, as the flagship kernel runs): v_perm_b32 alone,
// v_dot4_u32_u8 alone (eight independent chains per lane each), and the three compare sections fed the same counts 0..4 and
// random words; every result is summed into the output and the forms' sums must agree.  The sections run twice: on uniform
// pseudo-random counts (the worst case for bank conflicts of scattered 8-byte reads) and on the counts of a 512 x 512 lattice
// that the host brings to T_c with 300 checkerboard heat-bath sweeps, consecutive lanes on consecutive octets of a row as in the
// pair loop (neighbouring lanes often read the same entry).  The isa_* kernels are not timed: they hold one section each, for the
// listings in profiles/k1_pair_table_microbench.txt and k1_quad_table_microbench.txt.
//   hipcc --offload-arch=gfx950 -O3 -o tools/microbench_pair_table tools/microbench_pair_table.hip && tools/microbench_pair_table
//   hipcc --offload-arch=gfx950 -O3 -S --cuda-device-only -o microbench_pair_table.s tools/microbench_pair_table.hip   (the ISA)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <math.h>
#include <stdlib.h>

#include <vector>

#define CHECK(x)                                                    \
    do {                                                            \
        hipError_t e_ = (x);                                        \
        if (e_ != hipSuccess) {                                     \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); \
            exit(1);                                                \
        }                                                           \
    } while (0)

typedef short v2s __attribute__((ext_vector_type(2)));
static __device__ __forceinline__ uint32_t perm(uint32_t s0, uint32_t s1, uint32_t sel) { return __builtin_amdgcn_perm(s0, s1, sel); }
static __device__ __forceinline__ uint32_t subsat16(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(v2s, a), __builtin_bit_cast(v2s, b)));
}
static __device__ __forceinline__ uint32_t dot4(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_udot4(a, b, c, false); }

struct Tables {
    uint32_t t16[5];                      // (min(thr >> 16, 65535) ^ 0x8000) for up = 0..4
    uint32_t tblH0, tblH1, tblL0, tblL1;  // the same split into byte tables
};

struct Octet {
    uint32_t w[4], cnt_lo, cnt_hi;
};

// ---------------------------------------------------------------- the two sections
static __device__ __forceinline__ uint32_t section_perm(const Octet& o, uint32_t tH0, uint32_t tH1, uint32_t tL0, uint32_t tL1) {
    const uint32_t Hl = perm(tH1, tH0, o.cnt_lo), Ll = perm(tL1, tL0, o.cnt_lo);
    const uint32_t Hh = perm(tH1, tH0, o.cnt_hi), Lh = perm(tL1, tL0, o.cnt_hi);
    const uint32_t dx = subsat16(o.w[0], perm(Hl, Ll, 0x05010400u));
    const uint32_t dy = subsat16(o.w[1], perm(Hl, Ll, 0x07030602u));
    const uint32_t dz = subsat16(o.w[2], perm(Hh, Lh, 0x05010400u));
    const uint32_t dw = subsat16(o.w[3], perm(Hh, Lh, 0x07030602u));
    return dx + dy + dz + dw;
}

#define LDS_AS __attribute__((address_space(3)))
// tbl: LDS byte address of the table (a compile-time constant in the kernels below: it goes into the offset field)
static __device__ __forceinline__ uint32_t section_table(const Octet& o, uint32_t tbl, uint32_t w01, uint32_t w23) {
    const uint32_t i0 = dot4(o.cnt_lo, w01, 0u), i1 = dot4(o.cnt_lo, w23, 0u);
    const uint32_t i2 = dot4(o.cnt_hi, w01, 0u), i3 = dot4(o.cnt_hi, w23, 0u);
    const uint32_t dx = subsat16(o.w[0], *(const LDS_AS uint32_t*)(uintptr_t)(tbl + i0));
    const uint32_t dy = subsat16(o.w[1], *(const LDS_AS uint32_t*)(uintptr_t)(tbl + i1));
    const uint32_t dz = subsat16(o.w[2], *(const LDS_AS uint32_t*)(uintptr_t)(tbl + i2));
    const uint32_t dw = subsat16(o.w[3], *(const LDS_AS uint32_t*)(uintptr_t)(tbl + i3));
    return dx + dy + dz + dw;
}

// quad form: cnt8 = the counts of four sites scaled by 8; tbl: LDS byte address of the 625-entry table
static __device__ __forceinline__ uint32_t section_quad(const Octet& o, uint32_t tbl, uint32_t wq) {
    const uint32_t i0 = dot4(o.cnt_lo, wq, 0u), i1 = dot4(o.cnt_hi, wq, 0u);
    const uint64_t e0 = *(const LDS_AS uint64_t*)(uintptr_t)(tbl + i0), e1 = *(const LDS_AS uint64_t*)(uintptr_t)(tbl + i1);
    const uint32_t dx = subsat16(o.w[0], (uint32_t)e0);
    const uint32_t dy = subsat16(o.w[1], (uint32_t)(e0 >> 32));
    const uint32_t dz = subsat16(o.w[2], (uint32_t)e1);
    const uint32_t dw = subsat16(o.w[3], (uint32_t)(e1 >> 32));
    return dx + dy + dz + dw;
}

// pseudo-random inputs of NOCT octets per lane, made before the clock starts: counts 0..4 per byte, any bits for the words
constexpr int NOCT = 4;
static __device__ __forceinline__ uint32_t lcg(uint32_t& s) {
    s = s * 1664525u + 1013904223u;
    return s ^ (s >> 15);
}
static __device__ __forceinline__ uint32_t counts(uint32_t& s) {
    const uint32_t x = lcg(s);
    return (x & 0x01010101u) + ((x >> 1) & 0x01010101u) + ((x >> 2) & 0x01010101u) + ((x >> 3) & 0x01010101u);  // four bits of each byte
}
// cnts != nullptr: the counts come from a lattice instead, ncnt octets in row-major order; consecutive lanes take consecutive octets
// scale: what the counts are multiplied by (8 for the quad form)
static __device__ __forceinline__ void make_inputs(Octet in[NOCT], uint32_t seed, const uint2* cnts, uint32_t ncnt, uint32_t scale) {
    const uint32_t g = threadIdx.x + blockIdx.x * blockDim.x;
    uint32_t s = seed * 2654435761u + g * 40503u + 1u;
    for (int q = 0; q < NOCT; ++q) {
        for (int j = 0; j < 4; ++j) in[q].w[j] = lcg(s);
        in[q].cnt_lo = counts(s);
        in[q].cnt_hi = counts(s);
        if (cnts) {
            const uint2 c = cnts[(g + (uint32_t)q * 4096u) % ncnt];
            in[q].cnt_lo = c.x;
            in[q].cnt_hi = c.y;
        }
        in[q].cnt_lo *= scale;
        in[q].cnt_hi *= scale;
    }
}
// the loop must not lift a section out: its inputs are opaque in every trip (no instruction)
static __device__ __forceinline__ void opaque(Octet& o) {
    asm volatile("" : "+v"(o.w[0]), "+v"(o.w[1]), "+v"(o.w[2]), "+v"(o.w[3]), "+v"(o.cnt_lo), "+v"(o.cnt_hi));
}

static __device__ __forceinline__ void fill_table(uint32_t* tbl2, const Tables& T) {
    if (threadIdx.x < 25) tbl2[threadIdx.x] = T.t16[threadIdx.x % 5] | (T.t16[threadIdx.x / 5] << 16);
    __syncthreads();
}
// entry c0 + 5 c1 + 25 c2 + 125 c3 = the 16-bit fields t16(c0), t16(c1), t16(c2), t16(c3): two consecutive w words
static __device__ __forceinline__ void fill_table4(uint64_t* tbl4, const Tables& T) {
    for (uint32_t i = threadIdx.x; i < 625; i += blockDim.x) {
        const uint32_t lo = T.t16[i % 5] | (T.t16[i / 5 % 5] << 16), hi = T.t16[i / 25 % 5] | (T.t16[i / 125] << 16);
        tbl4[i] = (uint64_t)lo | ((uint64_t)hi << 32);
    }
    __syncthreads();
}

static __device__ __forceinline__ void finish(uint32_t* out, uint32_t acc, long long t0, long long t1) {
    out[threadIdx.x + blockIdx.x * blockDim.x] = acc;
    if (threadIdx.x == 0 && blockIdx.x == 0) out[gridDim.x * blockDim.x] = (uint32_t)(t1 - t0);
}

// FORM 0: the loop and the sums alone (what every form pays besides its section), 1: perm form, 2: table form, 3: quad form
// One static LDS array per kernel, so either table sits at LDS address 0.
template <int FORM>
__global__ __launch_bounds__(1024) void k_section(uint32_t* out, int iters, uint32_t seed, Tables T, const uint2* cnts, uint32_t ncnt) {
    __shared__ uint64_t tbl8[FORM == 3 ? 625 : 13];
    uint32_t* const tbl2 = reinterpret_cast<uint32_t*>(tbl8);
    if (FORM == 3) fill_table4(tbl8, T);
    else fill_table(tbl2, T);
    Octet in[NOCT];
    make_inputs(in, seed, cnts, ncnt, FORM == 3 ? 8u : 1u);
    uint32_t tH0 = T.tblH0, tH1 = T.tblH1, tL0 = T.tblL0, tL1 = T.tblL1;
    asm volatile("" : "+v"(tH0), "+v"(tH1), "+v"(tL0), "+v"(tL1));  // byte tables in VGPRs, as in the pair loop
    const uint32_t tbl = (uint32_t)(uintptr_t)(LDS_AS uint32_t*)tbl2;
    uint32_t acc = 0;
    const long long t0 = clock64();
#pragma unroll 1
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int q = 0; q < NOCT; ++q) {
            opaque(in[q]);
            if (FORM == 0) acc += in[q].w[0] + in[q].w[1] + in[q].w[2] + in[q].w[3];
            if (FORM == 1) acc += section_perm(in[q], tH0, tH1, tL0, tL1);
            if (FORM == 2) acc += section_table(in[q], tbl, 0x00001404u, 0x14040000u);
            if (FORM == 3) acc += section_quad(in[q], tbl, 0x7D190501u);
        }
    }
    const long long t1 = clock64();
    finish(out, acc, t0, t1);
}

// OP 0: v_perm_b32, 1: v_dot4_u32_u8; eight independent chains per lane
template <int OP>
__global__ __launch_bounds__(1024) void k_op(uint32_t* out, int iters, uint32_t seed, Tables T) {
    uint32_t x[8], s = seed + threadIdx.x;
    for (int j = 0; j < 8; ++j) x[j] = lcg(s);
    uint32_t b = T.tblH0, c = T.tblL0;
    asm volatile("" : "+v"(b), "+v"(c));
    const long long t0 = clock64();
#pragma unroll 1
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = OP == 0 ? perm(x[j], b, c) : dot4(x[j], b, c);
    }
    const long long t1 = clock64();
    uint32_t acc = 0;
    for (int j = 0; j < 8; ++j) acc += x[j];
    finish(out, acc, t0, t1);
}

// one section each, inputs from memory: for the ISA listing only
__global__ void isa_perm_section(uint32_t* out, const Octet* in, Tables T) {
    uint32_t tH0 = T.tblH0, tH1 = T.tblH1, tL0 = T.tblL0, tL1 = T.tblL1;
    asm volatile("" : "+v"(tH0), "+v"(tH1), "+v"(tL0), "+v"(tL1));
    out[threadIdx.x] = section_perm(in[threadIdx.x], tH0, tH1, tL0, tL1);
}
__global__ void isa_table_section(uint32_t* out, const Octet* in, Tables T) {
    __shared__ uint32_t tbl2[25];
    fill_table(tbl2, T);
    out[threadIdx.x] = section_table(in[threadIdx.x], (uint32_t)(uintptr_t)(LDS_AS uint32_t*)tbl2, 0x00001404u, 0x14040000u);
}

__global__ void isa_quad_section(uint32_t* out, const Octet* in, Tables T) {
    __shared__ uint64_t tbl4[625];
    fill_table4(tbl4, T);
    out[threadIdx.x] = section_quad(in[threadIdx.x], (uint32_t)(uintptr_t)(LDS_AS uint64_t*)tbl4, 0x7D190501u);
}

// the count octets of an L x L periodic lattice at T_c after `sweeps` checkerboard heat-bath sweeps from a random start: for each
// colour and row, the octets of that colour's sites in column order (8 same-colour sites of a row = one octet, a byte per site)
static std::vector<uint2> tc_counts(int L, int sweeps) {
    std::vector<int8_t> up((size_t)L * L);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return (double)(s >> 11) * (1.0 / 9007199254740992.0);
    };
    for (auto& u : up) u = rnd() < 0.5;
    const double beta = 0.5 * log(1.0 + sqrt(2.0));
    double p_up[5];
    for (int c = 0; c < 5; ++c) p_up[c] = 1.0 / (1.0 + exp(-2.0 * beta * (2 * c - 4)));
    auto nb = [&](int r, int c) {
        const int ru = (r + L - 1) % L, rd = (r + 1) % L, cl = (c + L - 1) % L, cr = (c + 1) % L;
        return up[(size_t)ru * L + c] + up[(size_t)rd * L + c] + up[(size_t)r * L + cl] + up[(size_t)r * L + cr];
    };
    for (int sw = 0; sw < sweeps; ++sw)
        for (int col = 0; col < 2; ++col)
            for (int r = 0; r < L; ++r)
                for (int c = (r + col) & 1; c < L; c += 2) up[(size_t)r * L + c] = rnd() < p_up[nb(r, c)];
    std::vector<uint2> out;
    for (int col = 0; col < 2; ++col)
        for (int r = 0; r < L; ++r)
            for (int o = 0; o < L / 16; ++o) {
                uint32_t w[2] = {0, 0};
                for (int j = 0; j < 8; ++j) w[j >> 2] |= (uint32_t)nb(r, 16 * o + 2 * j + ((r + col) & 1)) << (8 * (j & 3));
                out.push_back(make_uint2(w[0], w[1]));
            }
    return out;
}

int main() {
    const int iters = 4096, block = 1024;
    int dev = 0, cus = 0, khz = 0;
    CHECK(hipGetDevice(&dev));
    CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, dev));
    const int grid = cus;
    Tables T;
    // five distinct, asymmetric thresholds (both ends of the signed range among them)
    const uint32_t t16[5] = {0x0000u ^ 0x8000u, 0x1234u ^ 0x8000u, 0x7FFFu ^ 0x8000u, 0xC0DEu ^ 0x8000u, 0xFFFFu ^ 0x8000u};
    for (int c = 0; c < 5; ++c) T.t16[c] = t16[c];
    T.tblL0 = (t16[0] & 0xFF) | ((t16[1] & 0xFF) << 8) | ((t16[2] & 0xFF) << 16) | ((t16[3] & 0xFF) << 24);
    T.tblL1 = t16[4] & 0xFF;
    T.tblH0 = (t16[0] >> 8) | ((t16[1] >> 8) << 8) | ((t16[2] >> 8) << 16) | ((t16[3] >> 8) << 24);
    T.tblH1 = t16[4] >> 8;
    const size_t n = (size_t)grid * block;
    uint32_t* d;
    CHECK(hipMalloc(&d, (n + 1) * 4));
    uint32_t* h = (uint32_t*)malloc((n + 1) * 4);
    const std::vector<uint2> tc = tc_counts(512, 300);
    uint2* d_tc;
    CHECK(hipMalloc(&d_tc, tc.size() * sizeof(uint2)));
    CHECK(hipMemcpy(d_tc, tc.data(), tc.size() * sizeof(uint2), hipMemcpyHostToDevice));
    {  // how often each count occurs in the T_c lattice (uniform: 1/16, 4/16, 6/16, 4/16, 1/16 from four random bits)
        double hist[5] = {0, 0, 0, 0, 0};
        for (const uint2& c : tc)
            for (int j = 0; j < 8; ++j) hist[((j < 4 ? c.x : c.y) >> (8 * (j & 3))) & 0xFF] += 1.0 / (8.0 * tc.size());
        printf("T_c counts (512 x 512, 300 sweeps): P(0..4) = %.3f %.3f %.3f %.3f %.3f\n", hist[0], hist[1], hist[2], hist[3], hist[4]);
    }
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    printf("%d CUs, one %d-thread workgroup each (4 waves per SIMD), %d trips, clock %.0f MHz\n", cus, block, iters, khz / 1e3);
    const char* names[6] = {"v_perm_b32 alone (32 per trip)", "v_dot4_u32_u8 alone (32 per trip)", "loop and sums alone (4 octets per trip)",
                            "perm compare section (4 octets per trip)", "table compare section (4 octets per trip)",
                            "quad compare section (4 octets per trip)"};
    const int per_trip[6] = {32, 32, NOCT, NOCT, NOCT, NOCT};
    bool agree = true;
    for (int dist = 0; dist < 2; ++dist) {
        const uint2* cn = dist ? d_tc : nullptr;
        const uint32_t ncn = (uint32_t)tc.size();
        printf("---- %s\n", dist ? "counts of the lattice at T_c" : "uniform pseudo-random counts");
        double best_ms[6];
        uint64_t sums[6];
        for (int form = dist ? 2 : 0; form < 6; ++form) {
            double best = 1e30;
            for (int rep = 0; rep < 4; ++rep) {  // the first is the warm-up
                CHECK(hipEventRecord(e0));
                switch (form) {
                    case 0: k_op<0><<<grid, block>>>(d, iters, 12345u, T); break;
                    case 1: k_op<1><<<grid, block>>>(d, iters, 12345u, T); break;
                    case 2: k_section<0><<<grid, block>>>(d, iters, 12345u, T, cn, ncn); break;
                    case 3: k_section<1><<<grid, block>>>(d, iters, 12345u, T, cn, ncn); break;
                    case 4: k_section<2><<<grid, block>>>(d, iters, 12345u, T, cn, ncn); break;
                    default: k_section<3><<<grid, block>>>(d, iters, 12345u, T, cn, ncn); break;
                }
                CHECK(hipGetLastError());
                CHECK(hipEventRecord(e1));
                CHECK(hipDeviceSynchronize());
                float ms;
                CHECK(hipEventElapsedTime(&ms, e0, e1));
                if (rep > 0 && ms < best) best = ms;
            }
            CHECK(hipMemcpy(h, d, (n + 1) * 4, hipMemcpyDeviceToHost));
            const uint32_t ticks = h[n];
            uint64_t sum = 0;
            for (size_t i = 0; i < n; ++i) sum += h[i];
            sums[form] = sum;
            best_ms[form] = best;
            // a SIMD issues for its 4 waves in turn: time per unit and SIMD = kernel time / (trips x units per trip x 4 waves)
            const double ns = best * 1e6 / ((double)iters * per_trip[form] * 4);
            printf("%-44s kernel %.3f ms; %.3f ns = %.2f cycles per %s and wave on its SIMD; wave 0: %.1f clock64 ticks per trip; sum %016llx\n",
                   names[form], best, ns, ns * khz / 1e6, form < 2 ? "instruction" : "octet", (double)ticks / iters, (unsigned long long)sum);
        }
        const double base = best_ms[2], pm = best_ms[3] - base, tb = best_ms[4] - base, qd = best_ms[5] - base;
        printf("sections net of the loop and sums: perm %.3f ms, table %.3f ms, quad %.3f ms (table / perm = %.3f, quad / table = %.3f)\n", pm, tb,
               qd, tb / pm, qd / tb);
        const bool ok = sums[3] == sums[4] && sums[3] == sums[5];
        printf("sums of the three forms %s\n", ok ? "agree" : "DIFFER");
        agree = agree && ok;
    }
    return agree ? 0 : 1;
}

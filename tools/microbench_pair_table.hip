// microbench_pair_table.hip -- what does the compare section of the K1 pair loop (csrc/ising2d_tiled.hip) cost when the 16-bit
// thresholds of a site pair come from a 25-dword LDS table instead of v_perm_b32 byte look-ups?
//   perm form  (compare_octet today): 4 v_perm pick the high / low threshold bytes by the byte counts, 4 v_perm interleave them
//              into the 16-bit fields of v_pk_sub_i16: 8 v_perm + 4 v_pk_sub_i16 per octet
//   table form: v_dot4_u32_u8(cnt, weights, 0) with byte weights (4, 20, 0, 0) / (0, 0, 4, 20) is the byte offset 4 c0 + 20 c1 of the
//              dword t16(c0) | t16(c1) << 16 in a table of 25 dwords: 4 v_dot4 + 4 ds_read_b32 + 4 v_pk_sub_i16 per octet
// Four timed kernels, one 1024-thread workgroup per CU (4 waves per SIMD, as the flagship kernel runs): v_perm_b32 alone,
// v_dot4_u32_u8 alone (eight independent chains per lane each), and the two compare sections fed the same pseudo-random counts
// 0..4 and random words; every result is summed into the output and the two forms' sums must agree.  The two isa_* kernels are
// not timed: they hold one section each, for the listing in profiles/k1_pair_table_microbench.txt.
//   hipcc --offload-arch=gfx950 -O3 -o tools/microbench_pair_table tools/microbench_pair_table.hip && tools/microbench_pair_table
//   hipcc --offload-arch=gfx950 -O3 -S --cuda-device-only -o microbench_pair_table.s tools/microbench_pair_table.hip   (the ISA)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

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
static __device__ __forceinline__ void make_inputs(Octet in[NOCT], uint32_t seed) {
    uint32_t s = seed * 2654435761u + (threadIdx.x + blockIdx.x * blockDim.x) * 40503u + 1u;
    for (int q = 0; q < NOCT; ++q) {
        for (int j = 0; j < 4; ++j) in[q].w[j] = lcg(s);
        in[q].cnt_lo = counts(s);
        in[q].cnt_hi = counts(s);
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

static __device__ __forceinline__ void finish(uint32_t* out, uint32_t acc, long long t0, long long t1) {
    out[threadIdx.x + blockIdx.x * blockDim.x] = acc;
    if (threadIdx.x == 0 && blockIdx.x == 0) out[gridDim.x * blockDim.x] = (uint32_t)(t1 - t0);
}

// FORM 0: the loop and the sums alone (what both forms pay besides their section), 1: perm form, 2: table form
template <int FORM>
__global__ __launch_bounds__(1024) void k_section(uint32_t* out, int iters, uint32_t seed, Tables T) {
    __shared__ uint32_t tbl2[25];
    fill_table(tbl2, T);
    Octet in[NOCT];
    make_inputs(in, seed);
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
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    printf("%d CUs, one %d-thread workgroup each (4 waves per SIMD), %d trips, clock %.0f MHz\n", cus, block, iters, khz / 1e3);
    const char* names[5] = {"v_perm_b32 alone (32 per trip)", "v_dot4_u32_u8 alone (32 per trip)", "loop and sums alone (4 octets per trip)",
                            "perm compare section (4 octets per trip)", "table compare section (4 octets per trip)"};
    const int per_trip[5] = {32, 32, NOCT, NOCT, NOCT};
    double best_ms[5];
    uint64_t sums[5];
    for (int form = 0; form < 5; ++form) {
        double best = 1e30;
        uint32_t ticks = 0;
        for (int rep = 0; rep < 4; ++rep) {  // the first is the warm-up
            CHECK(hipEventRecord(e0));
            switch (form) {
                case 0: k_op<0><<<grid, block>>>(d, iters, 12345u, T); break;
                case 1: k_op<1><<<grid, block>>>(d, iters, 12345u, T); break;
                case 2: k_section<0><<<grid, block>>>(d, iters, 12345u, T); break;
                case 3: k_section<1><<<grid, block>>>(d, iters, 12345u, T); break;
                default: k_section<2><<<grid, block>>>(d, iters, 12345u, T); break;
            }
            CHECK(hipGetLastError());
            CHECK(hipEventRecord(e1));
            CHECK(hipDeviceSynchronize());
            float ms;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            if (rep > 0 && ms < best) best = ms;
        }
        CHECK(hipMemcpy(h, d, (n + 1) * 4, hipMemcpyDeviceToHost));
        ticks = h[n];
        uint64_t sum = 0;
        for (size_t i = 0; i < n; ++i) sum += h[i];
        sums[form] = sum;
        best_ms[form] = best;
        // a SIMD issues for its 4 waves in turn: time per unit and SIMD = kernel time / (trips x units per trip x 4 waves)
        const double ns = best * 1e6 / ((double)iters * per_trip[form] * 4);
        printf("%-44s kernel %.3f ms; %.3f ns = %.2f cycles per %s and wave on its SIMD; wave 0: %.1f clock64 ticks per trip; sum %016llx\n",
               names[form], best, ns, ns * khz / 1e6, form < 2 ? "instruction" : "octet", (double)ticks / iters, (unsigned long long)sum);
    }
    const double base = best_ms[2], pm = best_ms[3] - base, tb = best_ms[4] - base;
    printf("sections net of the loop and sums: perm %.3f ms, table %.3f ms (table / perm = %.3f)\n", pm, tb, tb / pm);
    printf("sums of the two forms %s\n", sums[3] == sums[4] ? "agree" : "DIFFER");
    return sums[3] == sums[4] ? 0 : 1;
}

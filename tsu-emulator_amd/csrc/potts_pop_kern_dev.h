// potts_pop_kern_dev.h -- the device side of K14, population annealing of K12's lattice (potts_pop.hip is the host side,
// potts_pop_plan.h the packing rule; DESIGN.md section 3, "Population annealing of Potts lattices (K14)").  R walkers on ONE disorder
// and ONE temperature; walker i is a whole K12 lattice at s + i stride of one allocation (stride = sites rounded up to 16 bytes, the
// pad bytes zero and never read here) with the Philox key seed + i.  The decision rule, the octet bodies and the measuring order are
// K12's (potts_disorder_kern_dev.h, used as they stand): a walker's colours and energy have the bits K12 gives the same lattice.  The
// resampling is pop_dev.h's pop_plan and pop_copy, unchanged; the final sums of a measuring pass are k13_pt_final's.
//   k14_pop_pack<DIM, HAS_H>          G >= 2 walkers a workgroup: lane l serves octet l % nlanes of walker l / nlanes of its group;
//                                     the group's colours in LDS for all sweeps of a step, the disorder staged in LDS once per
//                                     launch, pd_octet on LDS addresses; one launch per step for all walkers
//   k14_pop_small<DIM, HAS_H>         at most 16384 sites: one workgroup per walker (k13_pt_small's body)
//   k14_pop_sweep<DIM, ROWS16, HAS_H> one launch per half-sweep for all walkers, grid (k12_sweep's, walkers) (k13_pt_sweep's two paths)
//   k14_pop_measure<DIM, HAS_H>       grid (pd_measure_blocks, walkers): k13_pt_measure's lanes, order and tree at the walkers' stride
//   k14_pop_init                      grid (lanes, walkers): the device draw of init
#pragma once
#include "pop_dev.h"
#include "potts_pop_plan.h"
#include "potts_pt_kern_dev.h"

// Colour of the site whose 32-bit word of the init block is W: uniform in 0 .. q - 1 to within q 2^-32 (the cluster colours' rule)
POTTS_HD int potts_pop_draw(uint32_t W, int q) { return (int)(((uint64_t)W * (uint64_t)q) >> 32); }

namespace {

static_assert(kPopSmallSites == kPottsSmallSites && kPopSmallMaxThreads == kSwMaxThreads, "potts_pop_plan.h restates the one-workgroup limits");

struct PopWalkers {           // where walker i finds what is its own
    long long stride;         // bytes between two walkers' colours
    unsigned long long seed;  // walker i's key is seed + i
    int R;
};

// p, which describes walker 0, made walker i's; T is uniform and stays
template <int DIM>
__device__ __forceinline__ void ppop_select(PdSweep<DIM>& p, const PopWalkers& w, int i) {
    p.s += (long long)i * w.stride;
    const unsigned long long key = w.seed + (unsigned long long)i;
    p.k.k0 = (uint32_t)key;
    p.k.k1 = (uint32_t)(key >> 32);
}

// Workgroup b holds walkers b G .. b G + G - 1 (the last group fewer: its idle lanes reach every barrier and touch nothing).
// Dynamic LDS: the coupling planes, the q field planes (HAS_H), then G colour planes at the walkers' stride.  p.hs = the first sweep
template <int DIM, bool HAS_H>
__global__ __launch_bounds__(kPopPackThreads) void k14_pop_pack(PdSweep<DIM> p, PopWalkers w, int G, int n_sweeps) {
    extern __shared__ float s_dis[];
    const int nrows = (DIM == 3 ? p.g.depth : 1) * p.g.rows, n = nrows * p.g.cols;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int noct = (p.g.cols + 15) >> 4, nlanes = nrows * noct;
    constexpr int NJ = DIM == 2 ? 2 : 3;
    const int nf = HAS_H ? p.m.q * n : 0;
    int8_t* const s_sp = reinterpret_cast<int8_t*>(s_dis + NJ * n + nf);
    const int stride = (int)w.stride;
    const int first = (int)blockIdx.x * G, cnt = w.R - first < G ? w.R - first : G;
    int8_t* const gs = p.s + (long long)first * w.stride;
    for (int i = tid; i < n; i += nt) {
        s_dis[i] = p.m.jr[i];
        s_dis[n + i] = p.m.jd[i];
        if constexpr (DIM == 3) s_dis[2 * n + i] = p.m.jl[i];
    }
    if constexpr (HAS_H)
        for (int i = tid; i < nf; i += nt) s_dis[NJ * n + i] = p.m.h[i];  // colour-major, plane stride = sites = n
    for (int i = tid; i < cnt * n; i += nt) {
        const int g = i / n, j = i - g * n;
        s_sp[g * stride + j] = gs[(long long)g * w.stride + j];
    }
    __syncthreads();
    PdModel m = p.m;
    m.jr = s_dis;
    m.jd = s_dis + n;
    m.jl = DIM == 3 ? s_dis + 2 * n : nullptr;
    m.h = HAS_H ? s_dis + NJ * n : nullptr;
    const int g = tid / nlanes, l = tid - g * nlanes;
    const bool active = g < cnt;
    const int rho = l / noct, o = l - rho * noct;
    const unsigned long long key = w.seed + (unsigned long long)(first + g);
    const PottsKeys k = {(uint32_t)key, (uint32_t)(key >> 32), p.k.tag_hi, p.k.tag_lo};
    int8_t* const mine = s_sp + (active ? g : 0) * stride;
    for (int s = 0; s < n_sweeps; ++s) {
#pragma unroll 1
        for (int colour = 0; colour < 2; ++colour) {
            const uint32_t hs = 2u * (p.hs + (uint32_t)s) + (uint32_t)colour;
            if (active) pd_octet<DIM, HAS_H>(mine, p.g, m, k, hs, rho, o, colour);
            __syncthreads();
        }
    }
    for (int i = tid; i < cnt * n; i += nt) {
        const int g2 = i / n, j = i - g2 * n;
        gs[(long long)g2 * w.stride + j] = s_sp[g2 * stride + j];
    }
}

// k13_pt_small at the walkers' stride: blockIdx.x = walker, p.hs = the first sweep of the step
template <int DIM, bool HAS_H>
__global__ __launch_bounds__(kSwMaxThreads) void k14_pop_small(PdSweep<DIM> p, PopWalkers w, int n_sweeps) {
    __shared__ int8_t s_sp[kPottsSmallSites];
    ppop_select(p, w, (int)blockIdx.x);
    const int nrows = (DIM == 3 ? p.g.depth : 1) * p.g.rows, n = nrows * p.g.cols;  // n <= kPottsSmallSites: the host's route
    const int tid = threadIdx.x, nt = blockDim.x;
    const int noct = (p.g.cols + 15) >> 4, nlanes = nrows * noct;
    for (int i = tid; i < n; i += nt) s_sp[i] = p.s[i];
    __syncthreads();
    for (int s = 0; s < n_sweeps; ++s) {
#pragma unroll 1
        for (int colour = 0; colour < 2; ++colour) {
            const uint32_t hs = 2u * (p.hs + (uint32_t)s) + (uint32_t)colour;
            for (int l = tid; l < nlanes; l += nt) {
                const int rho = l / noct, o = l - rho * noct;
                pd_octet<DIM, HAS_H>(s_sp, p.g, p.m, p.k, hs, rho, o, colour);
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < n; i += nt) p.s[i] = s_sp[i];
}

// k13_pt_sweep at the walkers' stride: blockIdx.y = walker, p.hs = the half-sweep.  ROWS16: cols % 16 == 0, so stride = sites and
// every walker's rows stay 16-byte aligned
template <int DIM, bool ROWS16, bool HAS_H>
__global__ __launch_bounds__(256) void k14_pop_sweep(PdSweep<DIM> p, PopWalkers w) {
    const int noct = (p.g.cols + 15) >> 4;
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= (long long)(DIM == 3 ? p.g.depth : 1) * p.g.rows * noct) return;
    ppop_select(p, w, (int)blockIdx.y);
    const int rho = (int)(lane / noct), o = (int)(lane - (long long)rho * noct);
    const int colour = (int)(p.hs & 1u);
    if constexpr (!ROWS16) {
        pd_octet<DIM, HAS_H>(p.s, p.g, p.m, p.k, p.hs, rho, o, colour);
    } else {
        const int z = DIM == 3 ? rho / p.g.rows : 0, r = rho - z * p.g.rows;
        if (((z + r + colour) & 1) == 0) pd_octet_rows16<DIM, 0, HAS_H>(p.s, p.g, p.m, p.k, p.hs, z, r, o);
        else pd_octet_rows16<DIM, 1, HAS_H>(p.s, p.g, p.m, p.k, p.hs, z, r, o);
    }
}

// k13_pt_measure with walker blockIdx.y at p.s + blockIdx.y stride: the same lanes, the same order of a lane's sites and adds, the
// same grid in x and block_sum, so a walker's partials are the ones k12_measure writes for that lattice
template <int DIM, bool HAS_H>
__global__ __launch_bounds__(256) void k14_pop_measure(PtpMeasure p, long long stride) {
    __shared__ unsigned long long s_row[TSU_POTTS_RECORD_WORDS];
    if (threadIdx.x < TSU_POTTS_RECORD_WORDS) s_row[threadIdx.x] = 0;
    __syncthreads();
    const long long plane = (long long)p.g.rows * p.g.cols, n = plane * (DIM == 3 ? p.g.depth : 1);
    const int8_t* const s = p.s + (long long)blockIdx.y * stride;
    unsigned long long acc[TSU_POTTS_RECORD_WORDS] = {};  // wave-uniform
    double e = 0.0;
    for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {  // whole waves stay in
        const long long i = base + threadIdx.x;
        const bool valid = i < n;
        int col = -1;
        bool eq_r = false, eq_d = false, eq_l = false;
        if (valid) {
            const int z = DIM == 3 ? (int)(i / plane) : 0;
            const long long rem = i - (long long)z * plane;
            const int r = (int)(rem / p.g.cols), c = (int)(rem - (long long)r * p.g.cols);
            col = s[i];
            const int cr = c + 1 < p.g.cols ? c + 1 : (potts_pc<DIM>(p.g) ? 0 : -1);
            const int rd = r + 1 < p.g.rows ? r + 1 : (p.g.pr ? 0 : -1);
            eq_r = cr >= 0 && s[(long long)z * plane + (long long)r * p.g.cols + cr] == col;
            eq_d = rd >= 0 && s[(long long)z * plane + (long long)rd * p.g.cols + c] == col;
            if constexpr (DIM == 3) {
                const int zl = z + 1 < p.g.depth ? z + 1 : (p.g.pz ? 0 : -1);
                eq_l = zl >= 0 && s[(long long)zl * plane + rem] == col;
            }
            double l = 0.0;
            if constexpr (HAS_H) l = (double)p.m.h[(long long)col * p.m.sites + i];
            if (eq_r) l = __dadd_rn(l, (double)p.m.jr[i]);
            if (eq_d) l = __dadd_rn(l, (double)p.m.jd[i]);
            if constexpr (DIM == 3)
                if (eq_l) l = __dadd_rn(l, (double)p.m.jl[i]);
            e = __dadd_rn(e, l);
        }
        int n_eq = __popcll(__ballot(eq_r)) + __popcll(__ballot(eq_d));
        if constexpr (DIM == 3) n_eq += __popcll(__ballot(eq_l));
        acc[0] += (unsigned long long)n_eq;
#pragma unroll
        for (int c = 0; c < TSU_POTTS_MAX_Q; ++c)
            if (c < p.m.q) acc[1 + c] += (unsigned long long)__popcll(__ballot(col == c));
    }
    if ((threadIdx.x & 63u) == 0) {
#pragma unroll
        for (int k = 0; k < TSU_POTTS_RECORD_WORDS; ++k)
            if (acc[k] != 0) atomicAdd(&s_row[k], acc[k]);
    }
    const double be = block_sum(e);  // its barrier completes s_row as well
    const size_t at = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (threadIdx.x == 0) p.part[at] = be;
    if (threadIdx.x < TSU_POTTS_RECORD_WORDS) p.ipart[at * TSU_POTTS_RECORD_WORDS + threadIdx.x] = s_row[threadIdx.x];
}

// The device draw: lane (rho, o) of walker blockIdx.y writes the 16 columns of octet o of global row rho, four Philox blocks of four
// columns each: site (rho, c) = potts_pop_draw(word c & 3 of Philox(c >> 2, rho, 0, TAG_INIT), q), key = seed + walker
__global__ __launch_bounds__(256) void k14_pop_init(int8_t* __restrict__ s, PopWalkers w, int nrows, int cols, int q) {
    const int noct = (cols + 15) >> 4;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)nrows * noct) return;
    const int rho = (int)(t / noct), o = (int)(t - (long long)rho * noct);
    const unsigned long long key = w.seed + blockIdx.y;
    int8_t* const row = s + (long long)blockIdx.y * w.stride + (long long)rho * cols;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c0 = 16 * o + 4 * j;
        if (c0 >= cols) break;
        const u32x4 ph = tsu_philox((uint32_t)(c0 >> 2), (uint32_t)rho, 0u, TSU_TAG_INIT, (uint32_t)key, (uint32_t)(key >> 32));
        const uint32_t wv[4] = {ph.x, ph.y, ph.z, ph.w};
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (c0 + b < cols) row[c0 + b] = (int8_t)potts_pop_draw(wv[b], q);
    }
}

}  // namespace

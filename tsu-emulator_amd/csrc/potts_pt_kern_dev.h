// potts_pt_kern_dev.h -- the device side of K13, parallel tempering of K12's lattice (potts_pt.hip is the host side; DESIGN.md section 3,
// "Parallel tempering (K13)").  n_ladders ladders of R walkers on ONE disorder; walker g = ladder R + w is a whole K12 lattice at
// s + g sites of one allocation, with its own Philox key and the temperature of the slot it sits at.  The decision rule, the octet
// bodies and the measuring order are K12's (potts_disorder_kern_dev.h, used as they stand): a walker's colours and energy have the
// bits K12 gives the same lattice.  The swap pass is k7_pt_swap (pt_dev.h), filled through a PTSwap whose M column carries n_eq.
//   k13_pt_small<DIM, HAS_H>          at most 16384 sites: one workgroup per walker, its colours in LDS for all sweeps of a round, the
//                                     disorder through L2 (k12_small's body); one launch per round for all walkers
//   k13_pt_sweep<DIM, ROWS16, HAS_H>  one launch per half-sweep for all walkers, grid (k12_sweep's, walkers): k12_sweep's two paths.
//                                     A lane serves one walker: K12 is bound by its float64 exp, not by the disorder loads, so
//                                     nothing is gained by carrying several walkers over one load
//   k13_pt_measure<DIM, HAS_H>        grid (pd_measure_blocks, walkers): k12_measure's lanes, order and tree per walker, so E has
//                                     tsu_potts_dis_measure's bits; the integers as per-workgroup partials (no atomics, no zeroing)
//   k13_pt_final                      one workgroup per walker: E as energy_final sums it, n_eq and N_0 .. N_7
//   k13_pt_table                      grid (blocks, slots), two ladders: the contingency table C[a][b] of the walkers of ladder 0 and
//                                     ladder 1 at a slot, by wave ballots and integer atomics into a zeroed history row
//   k13_pt_gather                     the colour counts of the walker at every (ladder, slot) into the history row
#pragma once
#include "potts_disorder_kern_dev.h"
#include "pt_dev.h"

namespace {

struct PtpTables {        // where walker g finds what is its own
    const uint32_t* key;  // walker -> (k0, k1)
    const int32_t* slot;  // walker (= [ladder][w]) -> slot
    const double* T;      // slot -> T
};

// p, which describes walker 0 at slot 0, made walker g's
template <int DIM>
__device__ __forceinline__ void ptp_select(PdSweep<DIM>& p, const PtpTables& t, int g) {
    p.s += (long long)g * p.m.sites;
    p.k.k0 = t.key[2 * g];
    p.k.k1 = t.key[2 * g + 1];
    p.m.T = t.T[t.slot[g]];
}

// k12_small per walker: blockIdx.x = walker, p.hs = the first sweep of the round
template <int DIM, bool HAS_H>
__global__ __launch_bounds__(kSwMaxThreads) void k13_pt_small(PdSweep<DIM> p, PtpTables t, int n_sweeps) {
    __shared__ int8_t s_sp[kPottsSmallSites];
    ptp_select(p, t, (int)blockIdx.x);
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

// k12_sweep per walker: blockIdx.y = walker, p.hs = the half-sweep
template <int DIM, bool ROWS16, bool HAS_H>
__global__ __launch_bounds__(256) void k13_pt_sweep(PdSweep<DIM> p, PtpTables t) {
    const int noct = (p.g.cols + 15) >> 4;
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= (long long)(DIM == 3 ? p.g.depth : 1) * p.g.rows * noct) return;
    ptp_select(p, t, (int)blockIdx.y);
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

// ---------------------------------------------------------------- observables of every walker
struct PtpMeasure {
    const int8_t* s;           // walker 0
    PottsGeom g;
    PdModel m;                 // T is not read
    double* part;              // [walker][gridDim.x] partials of the energy sum
    unsigned long long* ipart; // [walker][gridDim.x][TSU_POTTS_RECORD_WORDS] partials of n_eq, N_0 .. N_7
};

// k12_measure per walker (blockIdx.y): the same lanes, the same order of a lane's sites and adds, the same grid in x and block_sum,
// so a walker's partials are the ones k12_measure writes for that lattice.  The integers leave as this workgroup's partial row
template <int DIM, bool HAS_H>
__global__ __launch_bounds__(256) void k13_pt_measure(PtpMeasure p) {
    __shared__ unsigned long long s_row[TSU_POTTS_RECORD_WORDS];
    if (threadIdx.x < TSU_POTTS_RECORD_WORDS) s_row[threadIdx.x] = 0;
    __syncthreads();
    const long long plane = (long long)p.g.rows * p.g.cols, n = plane * (DIM == 3 ? p.g.depth : 1);
    const int8_t* const s = p.s + (long long)blockIdx.y * n;
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

// one workgroup per walker: E[g] as energy_final sums the walker's n partials, n_eq[g] and N[g][0 .. 7] (exact, any order)
__global__ __launch_bounds__(256) void k13_pt_final(const double* __restrict__ part, const unsigned long long* __restrict__ ipart, int n,
                                                    double* __restrict__ E, long long* __restrict__ n_eq, long long* __restrict__ N) {
    __shared__ unsigned long long s_row[TSU_POTTS_RECORD_WORDS];
    const int g = blockIdx.x;
    if (threadIdx.x < TSU_POTTS_RECORD_WORDS) s_row[threadIdx.x] = 0;
    __syncthreads();
    // lane = (partial row, word): 28 rows of 9 words per pass of 252 lanes
    const int word = (int)threadIdx.x % TSU_POTTS_RECORD_WORDS, first = (int)threadIdx.x / TSU_POTTS_RECORD_WORDS;
    constexpr int kRows = 256 / TSU_POTTS_RECORD_WORDS;
    unsigned long long v = 0;
    if (first < kRows)
        for (int b = first; b < n; b += kRows) v += ipart[((size_t)g * n + b) * TSU_POTTS_RECORD_WORDS + word];
    if (v != 0) atomicAdd(&s_row[word], v);
    const double e = final_sum(part + (size_t)g * n, n);  // its barrier completes s_row as well
    if (threadIdx.x == 0) {
        E[g] = e;
        n_eq[g] = (long long)s_row[0];
    }
    if (threadIdx.x >= 1 && threadIdx.x < TSU_POTTS_RECORD_WORDS) N[(size_t)g * TSU_POTTS_MAX_Q + threadIdx.x - 1] = (long long)s_row[threadIdx.x];
}

// ---------------------------------------------------------------- the record of a round
// Two ladders, grid (blocks, R): slot blockIdx.y's table C[a][b] = the sites that show colour a in ladder 0's walker and b in ladder
// 1's walker there, added into out[slot][a q + b] (zeroed ahead of the run).  q^2 <= 64: lane l of a wave keeps the count of code
// l, taken from one ballot per code; a wave adds its counts into LDS, a workgroup into HBM, with integer atomics only
__global__ __launch_bounds__(256) void k13_pt_table(const int8_t* __restrict__ s, const int32_t* __restrict__ was, int R, long long sites,
                                                    int q, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s_tab[TSU_POTTS_MAX_Q * TSU_POTTS_MAX_Q];
    const int slot = blockIdx.y, nq = q * q, lane = (int)(threadIdx.x & 63u);
    if (threadIdx.x < TSU_POTTS_MAX_Q * TSU_POTTS_MAX_Q) s_tab[threadIdx.x] = 0;
    __syncthreads();
    const int8_t* const a = s + (long long)was[slot] * sites;
    const int8_t* const b = s + (long long)(R + was[R + slot]) * sites;
    unsigned long long mine = 0;
    for (long long base = (long long)blockIdx.x * 256; base < sites; base += (long long)gridDim.x * 256) {  // whole waves stay in
        const long long i = base + threadIdx.x;
        const int code = i < sites ? (int)a[i] * q + (int)b[i] : -1;
        for (int c = 0; c < nq; ++c) {
            const int cnt = __popcll(__ballot(code == c));
            if (lane == c) mine += (unsigned long long)cnt;
        }
    }
    if (lane < nq && mine != 0) atomicAdd(&s_tab[lane], mine);
    __syncthreads();
    if ((int)threadIdx.x < nq && s_tab[threadIdx.x] != 0) atomicAdd(&out[(size_t)slot * nq + threadIdx.x], s_tab[threadIdx.x]);
}

// hN[ladder][slot][0 .. 7] = N[walker at (ladder, slot)][0 .. 7]: one lane per word, n = ladders R 8 words
__global__ __launch_bounds__(256) void k13_pt_gather(const long long* __restrict__ N, const int32_t* __restrict__ was, int R, int n,
                                                     long long* __restrict__ hN) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const int ks = i / TSU_POTTS_MAX_Q, c = i - ks * TSU_POTTS_MAX_Q;  // ks = ladder R + slot
    const int g = (ks / R) * R + was[ks];
    hN[i] = N[(size_t)g * TSU_POTTS_MAX_Q + c];
}

}  // namespace

// potts_disorder_kern_dev.h -- the device side of K12, the q-state Potts lattice with per-bond couplings and per-site colour fields
// (potts_disorder.hip is the host side, potts_disorder_dev.h the decision rule).  The lattice, the visiting order, the octet and the
// site uniform are K10's (potts_kern_dev.h, whose geometry, keys, draw and row helpers are used as they stand): int8 colours,
// row-major, pitch = cols, global row rho = z R + r, colour (z + r + c) & 1, hs = 2 sweep + colour, one Philox block per octet, the
// lo16 block only for a site whose colour differs between lo16 = 0 and lo16 = 65535.  The kernels are templates over DIM; DIM = 2
// carries no z term, load or bond.
//
// Disorder: fp32 planes of the lattice's shape, the entry at a site the bond that leaves it in +c (jr), +r (jd), +z (jl); the field
// colour-major, h[c * sites + site], so that an octet's 16 columns of one colour are one run.  HAS_H = false reads no field plane.
//   k12_sweep<DIM, ROWS16, HAS_H>   one launch per half-sweep through HBM, one lane per octet.  ROWS16 (cols % 16 == 0): aligned
//                                   16-byte loads of the spin rows and float4 runs of the coupling and field planes, quad by quad;
//                                   any other width: bounds-checked scalar loads.  A missing neighbour's load goes to a valid
//                                   address and is never used
//   k12_small<DIM, HAS_H>           at most 16384 sites, the colours in LDS for all sweeps of a call, a barrier per half-sweep, the
//                                   disorder read through L2
//   k12_measure<DIM, HAS_H>         n_eq and N_0 .. N_7 as k10_measure counts them, and a workgroup's partial of
//                                   sum_bonds J_b [s_i = s_j] + sum_i h[s_i][i] in float64: lane = site, grid-stride, a fixed grid,
//                                   the fixed tree of reduce_dev.h; energy_final (reduce_dev.h) sums the partials and negates
//   k12_sw_small / k12_sw_local / k12_sw_merge / k12_sw_resolve   K10's Swendsen-Wang kernels with a bond policy that carries the
//                                   coupling: active iff the colours agree and u < floor(-expm1(-J_b / T) 2^32), evaluated per
//                                   satisfied bond; the union-find, the seams and the root chase are uf_dev.h's and sw_dev.h's
#pragma once
#include "potts_disorder_dev.h"
#include "potts_kern_dev.h"
#include "reduce_dev.h"

namespace {

struct PdModel {  // what the rule reads besides the colours
    const float* jr;
    const float* jd;
    const float* jl;  // DIM = 2: not read
    const float* h;   // HAS_H = false: not read
    long long sites;  // the stride between two colour planes of h
    double T;
    int q;
};

template <int DIM>
struct PdSweep {
    int8_t* s;
    PottsGeom g;
    PottsKeys k;
    uint32_t hs;  // k12_sweep: the half-sweep; k12_small: the first sweep of the call
    PdModel m;
};

// Site m of the octet (rho, o): its new colour from the neighbour colours nb (-1: none), their couplings J and the field hv
template <int NB, bool HAS_H>
__device__ __forceinline__ int pd_site(const PdModel& md, const PottsKeys& k, uint32_t hs, int rho, int o, int m, const int (&nb)[NB],
                                       const float (&J)[NB], const float (&hv)[TSU_POTTS_MAX_Q], PottsDraw& d) {
    uint64_t thr[TSU_POTTS_MAX_Q];
    pd_site_thresholds<NB, HAS_H>(md.q, md.T, nb, J, hv, thr);
    const uint32_t hi = half_of(d.h0, d.h1, d.h2, d.h3, m) ^ 0x8000u;
    int col = pd_pick(thr, hi << 16);
    if (col != pd_pick(thr, (hi << 16) | 0xFFFFu)) {  // the low half decides: K1's lo16 block
        if (!d.have_lo) {
            const u32x4 l = tsu_philox((uint32_t)o, (uint32_t)rho, hs, k.tag_lo, k.k0, k.k1);
            d.l0 = l.x;
            d.l1 = l.y;
            d.l2 = l.z;
            d.l3 = l.w;
            d.have_lo = true;
        }
        col = pd_pick(thr, (hi << 16) | half_of(d.l0, d.l1, d.l2, d.l3, m));
    }
    return col;
}

// One colour of the octet (rho, o) by scalar loads: s the lattice in HBM or LDS, pitch = cols; the disorder in HBM.  Every index
// stays inside [0, depth rows cols): a missing neighbour is not loaded and its coupling is 0
template <int DIM, bool HAS_H>
__device__ __forceinline__ void pd_octet(int8_t* s, const PottsGeom& g, const PdModel& md, const PottsKeys& k, uint32_t hs, int rho, int o,
                                         int colour) {
    const int z = DIM == 3 ? rho / g.rows : 0, r = rho - z * g.rows;
    const int par = (z + r + colour) & 1, c0 = 16 * o;
    const PottsRows n = potts_rows<DIM>(g, z, r);
    const long long row = (long long)rho * g.cols;
    PottsDraw d = potts_draw(k, hs, rho, o);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int c = c0 + 2 * m + par;
        if (c >= g.cols) break;
        const int cl = c > 0 ? c - 1 : (potts_pc<DIM>(g) ? g.cols - 1 : -1);
        const int cr = c + 1 < g.cols ? c + 1 : (potts_pc<DIM>(g) ? 0 : -1);
        int nb[2 * DIM];  // DIM = 3: the layers first
        float J[2 * DIM];
        if constexpr (DIM == 3) {
            nb[0] = n.rzm >= 0 ? s[(long long)n.rzm * g.cols + c] : -1;
            J[0] = n.rzm >= 0 ? md.jl[(long long)n.rzm * g.cols + c] : 0.0f;
            nb[1] = n.rzp >= 0 ? s[(long long)n.rzp * g.cols + c] : -1;
            J[1] = n.rzp >= 0 ? md.jl[row + c] : 0.0f;
        }
        nb[2 * DIM - 4] = n.ru >= 0 ? s[(long long)n.ru * g.cols + c] : -1;
        J[2 * DIM - 4] = n.ru >= 0 ? md.jd[(long long)n.ru * g.cols + c] : 0.0f;
        nb[2 * DIM - 3] = n.rd >= 0 ? s[(long long)n.rd * g.cols + c] : -1;
        J[2 * DIM - 3] = n.rd >= 0 ? md.jd[row + c] : 0.0f;
        nb[2 * DIM - 2] = cl >= 0 ? s[row + cl] : -1;
        J[2 * DIM - 2] = cl >= 0 ? md.jr[row + cl] : 0.0f;
        nb[2 * DIM - 1] = cr >= 0 ? s[row + cr] : -1;
        J[2 * DIM - 1] = cr >= 0 ? md.jr[row + c] : 0.0f;
        float hv[TSU_POTTS_MAX_Q] = {};
        if constexpr (HAS_H) {
#pragma unroll
            for (int q = 0; q < TSU_POTTS_MAX_Q; ++q)
                if (q < md.q) hv[q] = md.h[(long long)q * md.sites + row + c];
        }
        s[row + c] = (int8_t)pd_site<2 * DIM, HAS_H>(md, k, hs, rho, o, m, nb, J, hv, d);
    }
}

// element k (0 .. 3) of a float4
__device__ __forceinline__ float f4at(const float4& v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : (k == 2 ? v.z : v.w)); }

// The same half-sweep of an octet of a lattice whose rows are whole octets (cols % 16 == 0: every 16-byte row segment is aligned and
// holds sites only, every run of 16 floats is four aligned float4): the spin rows as in potts_octet_rows16, the couplings and the
// field quad by quad (four columns, two of them of this colour), so that no more than one quad of every plane is live.  PAR = the
// parity of the colour's columns in this row
template <int DIM, int PAR, bool HAS_H>
__device__ __forceinline__ void pd_octet_rows16(int8_t* s, const PottsGeom& g, const PdModel& md, const PottsKeys& k, uint32_t hs, int z,
                                                int r, int o) {
    const int c0 = 16 * o, rho = (DIM == 3 ? z * g.rows : 0) + r;
    const PottsRows n = potts_rows<DIM>(g, z, r);
    const long long row = (long long)rho * g.cols;
    // a missing row or layer is loaded from this row (a valid address, no branch); what it brings is never used
    const long long rowu = (long long)(n.ru >= 0 ? n.ru : rho) * g.cols, rowd = (long long)(n.rd >= 0 ? n.rd : rho) * g.cols;
    const long long rowa = DIM == 3 ? (long long)(n.rzm >= 0 ? n.rzm : rho) * g.cols : 0;
    const long long rowb = DIM == 3 ? (long long)(n.rzp >= 0 ? n.rzp : rho) * g.cols : 0;
    const uint4 C = *reinterpret_cast<const uint4*>(s + row + c0);
    const uint4 U = *reinterpret_cast<const uint4*>(s + rowu + c0);
    const uint4 D = *reinterpret_cast<const uint4*>(s + rowd + c0);
    uint4 A = {}, B = {};
    if constexpr (DIM == 3) {
        A = *reinterpret_cast<const uint4*>(s + rowa + c0);
        B = *reinterpret_cast<const uint4*>(s + rowb + c0);
    }
    // the one neighbour outside the 16 bytes: left of position 0 (PAR = 0) or right of position 15 (PAR = 1).  Only the left one
    // brings a coupling from outside the run (the right bond of position 15 is stored at position 15)
    const int pc = potts_pc<DIM>(g);
    const int ce = PAR == 0 ? (c0 > 0 ? c0 - 1 : (pc ? g.cols - 1 : -1)) : (c0 + 16 < g.cols ? c0 + 16 : (pc ? 0 : -1));
    const int s_edge = ce >= 0 ? (int)s[row + ce] : -1;
    float j_left = PAR == 0 ? md.jr[row + (ce >= 0 ? ce : c0)] : 0.0f;  // the coupling to the left of the quad's first position
    PottsDraw d = potts_draw(k, hs, rho, o);
    uint32_t o0 = C.x, o1 = C.y, o2 = C.z, o3 = C.w;
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
        const int cq = c0 + 4 * qd;
        const float4 R = *reinterpret_cast<const float4*>(md.jr + row + cq);
        const float4 Dn = *reinterpret_cast<const float4*>(md.jd + row + cq);
        const float4 Up = *reinterpret_cast<const float4*>(md.jd + rowu + cq);
        float4 Fw = {}, Bk = {};
        if constexpr (DIM == 3) {
            Fw = *reinterpret_cast<const float4*>(md.jl + row + cq);
            Bk = *reinterpret_cast<const float4*>(md.jl + rowa + cq);
        }
        float4 H[TSU_POTTS_MAX_Q] = {};
        if constexpr (HAS_H) {
#pragma unroll
            for (int q = 0; q < TSU_POTTS_MAX_Q; ++q)
                if (q < md.q) H[q] = *reinterpret_cast<const float4*>(md.h + (long long)q * md.sites + row + cq);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int e = 2 * j + PAR, i = 4 * qd + e, m = 2 * qd + j;
            int nb[2 * DIM];
            float J[2 * DIM];
            if constexpr (DIM == 3) {
                nb[0] = n.rzm >= 0 ? colour_at(A, i) : -1;
                J[0] = f4at(Bk, e);
                nb[1] = n.rzp >= 0 ? colour_at(B, i) : -1;
                J[1] = f4at(Fw, e);
            }
            nb[2 * DIM - 4] = n.ru >= 0 ? colour_at(U, i) : -1;
            J[2 * DIM - 4] = f4at(Up, e);
            nb[2 * DIM - 3] = n.rd >= 0 ? colour_at(D, i) : -1;
            J[2 * DIM - 3] = f4at(Dn, e);
            nb[2 * DIM - 2] = i > 0 ? colour_at(C, i - 1) : s_edge;
            J[2 * DIM - 2] = e > 0 ? f4at(R, e - 1) : j_left;
            nb[2 * DIM - 1] = i < 15 ? colour_at(C, i + 1) : s_edge;
            J[2 * DIM - 1] = f4at(R, e);
            float hv[TSU_POTTS_MAX_Q] = {};
            if constexpr (HAS_H) {
#pragma unroll
                for (int q = 0; q < TSU_POTTS_MAX_Q; ++q) hv[q] = f4at(H[q], e);
            }
            const uint32_t col = (uint32_t)pd_site<2 * DIM, HAS_H>(md, k, hs, rho, o, m, nb, J, hv, d);
            const int sh = 8 * (i & 3);
            uint32_t& w = qd == 0 ? o0 : (qd == 1 ? o1 : (qd == 2 ? o2 : o3));
            w = (w & ~(0xFFu << sh)) | (col << sh);
        }
        j_left = R.w;
    }
    *reinterpret_cast<uint4*>(s + row + c0) = make_uint4(o0, o1, o2, o3);
}

template <int DIM, bool ROWS16, bool HAS_H>
__global__ __launch_bounds__(256) void k12_sweep(PdSweep<DIM> p) {
    const int noct = (p.g.cols + 15) >> 4;
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    if (lane >= (long long)(DIM == 3 ? p.g.depth : 1) * p.g.rows * noct) return;
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

template <int DIM, bool HAS_H>
__global__ __launch_bounds__(kSwMaxThreads) void k12_small(PdSweep<DIM> p, int n_sweeps) {
    __shared__ int8_t s_sp[kPottsSmallSites];
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

// ---------------------------------------------------------------- observables
struct PdMeasure {
    const int8_t* s;
    PottsGeom g;
    PdModel m;                // T is not read; jr == nullptr: no disorder set, the partials are 0
    unsigned long long* row;  // 9 words, zeroed on the stream ahead of the launch
    double* part;             // gridDim.x partials of the energy sum
};

// The integers exactly as k10_measure adds them.  The energy: lane = site, the lane's sites in rising order, a site adds
// l = h[s_i][i] (0.0 without a field), then + J_right, + J_down, + J_layer of its bonds that exist and join two equal colours; the
// workgroup's partial by block_sum.  The grid is a function of the shape alone (pd_measure_blocks), so E has the same bits on every
// call and every route
template <int DIM, bool HAS_H>
__global__ __launch_bounds__(256) void k12_measure(PdMeasure p) {
    __shared__ unsigned long long s_row[TSU_POTTS_RECORD_WORDS];
    if (threadIdx.x < TSU_POTTS_RECORD_WORDS) s_row[threadIdx.x] = 0;
    __syncthreads();
    const long long plane = (long long)p.g.rows * p.g.cols, n = plane * (DIM == 3 ? p.g.depth : 1);
    unsigned long long acc[TSU_POTTS_RECORD_WORDS] = {};  // wave-uniform: every lane of a wave holds the wave's counts
    double e = 0.0;
    const bool dis = p.m.jr != nullptr;
    for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {  // whole waves stay in
        const long long i = base + threadIdx.x;
        const bool valid = i < n;
        int col = -1;
        bool eq_r = false, eq_d = false, eq_l = false;
        if (valid) {
            const int z = DIM == 3 ? (int)(i / plane) : 0;
            const long long rem = i - (long long)z * plane;
            const int r = (int)(rem / p.g.cols), c = (int)(rem - (long long)r * p.g.cols);
            col = p.s[i];
            const int cr = c + 1 < p.g.cols ? c + 1 : (potts_pc<DIM>(p.g) ? 0 : -1);
            const int rd = r + 1 < p.g.rows ? r + 1 : (p.g.pr ? 0 : -1);
            eq_r = cr >= 0 && p.s[(long long)z * plane + (long long)r * p.g.cols + cr] == col;
            eq_d = rd >= 0 && p.s[(long long)z * plane + (long long)rd * p.g.cols + c] == col;
            if constexpr (DIM == 3) {
                const int zl = z + 1 < p.g.depth ? z + 1 : (p.g.pz ? 0 : -1);
                eq_l = zl >= 0 && p.s[(long long)zl * plane + rem] == col;
            }
            if (dis) {
                double l = 0.0;
                if constexpr (HAS_H) l = (double)p.m.h[(long long)col * p.m.sites + i];
                if (eq_r) l = __dadd_rn(l, (double)p.m.jr[i]);
                if (eq_d) l = __dadd_rn(l, (double)p.m.jd[i]);
                if constexpr (DIM == 3)
                    if (eq_l) l = __dadd_rn(l, (double)p.m.jl[i]);
                e = __dadd_rn(e, l);
            }
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
    if (threadIdx.x == 0) p.part[blockIdx.x] = be;
    if (threadIdx.x < TSU_POTTS_RECORD_WORDS && s_row[threadIdx.x] != 0) atomicAdd(&p.row[threadIdx.x], s_row[threadIdx.x]);
}

// ---------------------------------------------------------------- Swendsen-Wang steps on the stored couplings
struct PdBonds {  // the bond policy: two equal colours and u < thr(J_b, T), J_b >= 0 read where the bond leaves its site
    const float* jr;
    const float* jd;
    const float* jl;
    double T;
    int q;
    __device__ __forceinline__ static bool sat(int sa, int sb) { return sa == sb; }
    __device__ __forceinline__ bool below(float J, uint32_t u) const { return (uint64_t)u < pd_bond_threshold(J, T); }
    __device__ __forceinline__ bool on(float J, int sa, int sb, uint32_t u) const { return sa == sb && below(J, u); }
};

using PdItem = SwItem<PdBonds>;
using PdParams = SwParams<PdBonds>;

// k10_sw_small with the coupling of every satisfied bond read at global index i (the lattice is row 0 .. of one allocation)
template <int DIM, class... Rec>
__global__ __launch_bounds__(kSwMaxThreads) void k12_sw_small(const PdItem* __restrict__ items, PdItem one, SwGeom g, int n_steps, int* err,
                                                              Rec...) {
    extern __shared__ int s_lab[];
    __shared__ int s_bad;
    const PdItem& it = items ? items[blockIdx.x] : one;
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    const int rows = g.rows, cols = g.cols, pr = g.pr, pc = potts_pc<DIM>(g);
    const int nrows = (DIM == 3 ? g.depth : 1) * rows, n = nrows * cols, tid = threadIdx.x, nt = blockDim.x;
    int8_t* const s_spin = reinterpret_cast<int8_t*>(s_lab + n);
    if (tid == 0) s_bad = 0;
    for (int i = tid; i < n; i += nt) s_spin[i] = it.s[i];
    const int hc = (cols + 1) >> 1, npairs = nrows * hc;
    for (int s = 0; s < n_steps; ++s) {
        const uint32_t t = it.k.t + (uint32_t)s;
        for (int i = tid; i < n; i += nt) s_lab[i] = i;
        __syncthreads();
        int budget = kBudget;
        for (int p = tid; p < npairs; p += nt) {
            const int rho = p / hc, cp = p - rho * hc;
            const int z = DIM == 3 ? rho / rows : 0, r = rho - z * rows;
            const u32x4 w = tsu_philox((uint32_t)cp, (uint32_t)rho, t, it.k.tag_bond, it.k.k0, it.k.k1);
            const int rd = r + 1 < rows ? rho + 1 : (pr ? z * rows : -1);  // global row of the down neighbour
            [[maybe_unused]] int rf = -1;
            if constexpr (DIM == 3) rf = z + 1 < g.depth ? rho + rows : (g.pz ? r : -1);
            [[maybe_unused]] u32x4 wl = {0u, 0u, 0u, 0u};
            [[maybe_unused]] bool have_wl = false;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = 2 * cp + j;
                if (c >= cols) break;
                const int i = rho * cols + c, si = s_spin[i];
                const int cr = c + 1 < cols ? c + 1 : (pc ? 0 : -1);
                if (cr >= 0 && PdBonds::sat(si, s_spin[rho * cols + cr]) && it.b.below(it.b.jr[i], j ? w.z : w.x))
                    if (!uf_union<false, WG>(s_lab, i, rho * cols + cr, budget)) s_bad = 1;
                if (rd >= 0 && PdBonds::sat(si, s_spin[rd * cols + c]) && it.b.below(it.b.jd[i], j ? w.w : w.y))
                    if (!uf_union<false, WG>(s_lab, i, rd * cols + c, budget)) s_bad = 1;
                if constexpr (DIM == 3) {
                    if (rf >= 0 && PdBonds::sat(si, s_spin[rf * cols + c])) {
                        if (!have_wl) wl = tsu_philox((uint32_t)cp >> 1, (uint32_t)rho, t, it.k.tag_layer, it.k.k0, it.k.k1);
                        have_wl = true;
                        if (it.b.below(it.b.jl[i], word_of(wl, c & 3)))
                            if (!uf_union<false, WG>(s_lab, i, rf * cols + c, budget)) s_bad = 1;
                    }
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < n; i += nt) {
            budget = kBudget;
            const int root = uf_find<false, WG>(s_lab, i, budget);
            if (budget < 0) s_bad = 1;
            const int rr = root / cols, rc = root - rr * cols;
            s_spin[i] = (int8_t)root_colour(rr, rc, it.b.q, t, it.k.tag_flip, it.k.k0, it.k.k1);
        }
        __syncthreads();
        if (s_bad) break;
    }
    if (s_bad) {
        if (tid == 0) raise_err(err);
        return;  // the lattice keeps its colours from before the call
    }
    for (int i = tid; i < n; i += nt) it.s[i] = s_spin[i];
}

// k10_sw_local with stored couplings; the host's lane count (up to 1024) in both dimensions
template <int DIM>
__global__ __launch_bounds__(kSwMaxThreads) void k12_sw_local(PdParams p) {
    extern __shared__ int s_lab[];
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    const int TZ = DIM == 3 ? p.g.tz : 1, TR = p.g.tr, TC = p.g.tc, n = TZ * TR * TC;
    int8_t* const s_spin = reinterpret_cast<int8_t*>(s_lab + n);
    const int bz = DIM == 3 ? (int)(blockIdx.x / (unsigned)(p.g.nr * p.g.nc)) : 0, brc = (int)blockIdx.x - bz * p.g.nr * p.g.nc;
    const int br = brc / p.g.nc, bc = brc - br * p.g.nc;
    const int z0 = bz * TZ, r0 = br * TR, c0 = bc * TC;
    const int tz = DIM == 3 ? (p.g.depth - z0 < TZ ? p.g.depth - z0 : TZ) : 1;
    const int tr = p.g.rows - r0 < TR ? p.g.rows - r0 : TR, tc = p.g.cols - c0 < TC ? p.g.cols - c0 : TC;
    const int tid = threadIdx.x, nt = (int)blockDim.x;
    for (int i = tid; i < n; i += nt) {
        const int lz = DIM == 3 ? i / (TR * TC) : 0, rem = i - lz * TR * TC, lr = rem / TC, lc = rem - lr * TC;
        const long long rho = (long long)(z0 + lz) * p.g.rows + r0 + lr;
        s_lab[i] = i;
        s_spin[i] = (lz < tz && lr < tr && lc < tc) ? p.s[rho * p.g.pitch + c0 + lc] : (int8_t)-1;  // outside: no colour
    }
    __syncthreads();
    int budget = kBudget;
    bool bad = false;
    const int hw = TC >> 1;
    for (int q = tid; q < TZ * TR * hw; q += nt) {
        const int lz = DIM == 3 ? q / (TR * hw) : 0, rem = q - lz * TR * hw, lr = rem / hw, lc0 = 2 * (rem - lr * hw);
        if (lz >= tz || lr >= tr || lc0 >= tc) continue;
        const long long rho = (long long)(z0 + lz) * p.g.rows + r0 + lr;
        const u32x4 w = tsu_philox((uint32_t)(c0 + lc0) >> 1, (uint32_t)rho, p.k.t, p.k.tag_bond, p.k.k0, p.k.k1);
        [[maybe_unused]] u32x4 wl = {0u, 0u, 0u, 0u};
        [[maybe_unused]] bool have_wl = false;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int lc = lc0 + j;
            if (lc >= tc) break;
            const int i = (lz * TR + lr) * TC + lc, si = s_spin[i];
            const long long gi = rho * p.g.cols + c0 + lc;  // the site's global index: where its bonds' couplings are stored
            if (lc + 1 < tc && PdBonds::sat(si, s_spin[i + 1]) && p.b.below(p.b.jr[gi], j ? w.z : w.x))
                bad |= !uf_union<false, WG>(s_lab, i, i + 1, budget);
            if (lr + 1 < tr && PdBonds::sat(si, s_spin[i + TC]) && p.b.below(p.b.jd[gi], j ? w.w : w.y))
                bad |= !uf_union<false, WG>(s_lab, i, i + TC, budget);
            if constexpr (DIM == 3) {
                if (lz + 1 < tz && PdBonds::sat(si, s_spin[i + TR * TC])) {
                    if (!have_wl) wl = tsu_philox((uint32_t)(c0 + lc0) >> 2, (uint32_t)rho, p.k.t, p.k.tag_layer, p.k.k0, p.k.k1);
                    have_wl = true;
                    if (p.b.below(p.b.jl[gi], word_of(wl, (c0 + lc) & 3))) bad |= !uf_union<false, WG>(s_lab, i, i + TR * TC, budget);
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += nt) {
        const int lz = DIM == 3 ? i / (TR * TC) : 0, rem = i - lz * TR * TC, lr = rem / TC, lc = rem - lr * TC;
        if (lz >= tz || lr >= tr || lc >= tc) continue;
        budget = kBudget;
        const int root = uf_find<false, WG>(s_lab, i, budget);
        bad |= budget < 0;
        const int rz = DIM == 3 ? root / (TR * TC) : 0, rrem = root - rz * TR * TC, rr = rrem / TC, rc = rrem - rr * TC;
        const long long rho = (long long)(z0 + lz) * p.g.rows + r0 + lr;
        p.labels[rho * p.g.cols + c0 + lc] = ((z0 + rz) * p.g.rows + r0 + rr) * p.g.cols + c0 + rc;
    }
    if (bad) raise_err(p.err);
}

// one lane per bond across a tile face or a wrap (sw_seam); the bond leaves (rho, c) along `axis`
template <int DIM>
__global__ __launch_bounds__(256) void k12_sw_merge(PdParams p) {
    sw_row_t<DIM> rho, rho2;
    int c, c2;
    const int axis = sw_seam<DIM>(p.g, (long long)blockIdx.x * 256 + threadIdx.x, rho, c, rho2, c2);
    if (axis < 0) return;
    const int sa = p.s[(long long)rho * p.g.pitch + c], sb = p.s[(long long)rho2 * p.g.pitch + c2];
    if (!PdBonds::sat(sa, sb)) return;
    const long long gi = (long long)rho * p.g.cols + c;
    uint32_t u;
    float J;
    if (DIM == 3 && axis == 2) {
        u = word_of(tsu_philox((uint32_t)c >> 2, (uint32_t)rho, p.k.t, p.k.tag_layer, p.k.k0, p.k.k1), c & 3);
        J = p.b.jl[gi];
    } else {
        const u32x4 w = tsu_philox((uint32_t)c >> 1, (uint32_t)rho, p.k.t, p.k.tag_bond, p.k.k0, p.k.k1);
        u = word_of(w, 2 * (c & 1) + axis);
        J = axis ? p.b.jd[gi] : p.b.jr[gi];
    }
    if (!p.b.below(J, u)) return;
    int budget = kBudget;
    const int a = p.labels[gi], b = p.labels[(long long)rho2 * p.g.cols + c2];
    if (!uf_union<false, __HIP_MEMORY_SCOPE_AGENT>(p.labels, a, b, budget)) raise_err(p.err);
}

// k10_sw_resolve on this policy's parameters: one lane per 4 sites of a global row, the root's colour stored as a byte
template <int DIM>
__global__ __launch_bounds__(256) void k12_sw_resolve(PdParams p, int quads) {
    const SwGeom& g = p.g;
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    const sw_row_t<DIM> rho = (sw_row_t<DIM>)(lane / quads);
    const int c0 = 4 * (int)(lane - (long long)rho * quads);
    if (rho >= (sw_row_t<DIM>)(DIM == 3 ? g.depth : 1) * g.rows) return;
    int last = -1, last_colour = 0;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (c0 + j >= g.cols) break;
        const int x = sw_chase<false>(p.labels, p.labels[(long long)rho * g.cols + c0 + j], bad);
        if (x != last) {
            const int rr = x / g.cols, rc = x - rr * g.cols;
            last = x;
            last_colour = root_colour(rr, rc, p.b.q, p.k.t, p.k.tag_flip, p.k.k0, p.k.k1);
        }
        p.s[(long long)rho * g.pitch + c0 + j] = (int8_t)last_colour;
    }
    if (bad) raise_err(p.err);
}

}  // namespace

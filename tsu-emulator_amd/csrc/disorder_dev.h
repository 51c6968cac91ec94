// disorder_dev.h -- what the heat-bath kernels with per-bond couplings share on the device: K7 (ising2d_disorder.hip, 2-D) and K8
// (ising3d.hip, 3-D), single lattices, tempering ladders, ensembles and populations alike.  The decision rule of the contract
//  is written once, in Octet: an fp32 screen first, the float64 threshold only where the screen cannot
// decide, the lo16 Philox block only on a tie.  Also here: the structs the kernels take (Geo, Walker, PTParams, PTEns) and the one
// energy lane.  The __global__ kernels, their lane mappings and their grids stay with their dimension.
#pragma once
#include <cmath>

#include "tsu_common.h"

// byte i (0 .. 15) of a 16-byte load, sign-extended: spin i of an octet's 16 columns
__device__ __forceinline__ int sbyte(const uint4& v, int i) {
    const uint32_t w = i < 4 ? v.x : (i < 8 ? v.y : (i < 12 ? v.z : v.w));
    return (int)(int8_t)((w >> (8 * (i & 3))) & 0xFFu);
}

// element i (0 .. 15) of 16 consecutive floats held as four float4
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
// |terms|, A = 2 S / T and n fp32 additions in the field (the products J s are exact, s = +-1):  the additions err by
// <= n u S; times fl(2 / T) adds 2 u |x|: |dx| <= (n + 3) u A.  __expf(-x) is v_exp_f32 of fl(-x fl32(log2 e)): the constant
// is 0.23 u short and the product rounds by u, 1.23 |x| u relative after the exponential, and v_exp_f32 adds 1 ulp <= 2 u:
// (1.23 |x| + 2) u, with 3 u for the add and rcp.  The device stays inside both over the fp32 range (tsu_probe_screen,
// tests/test_screen_gpu.py, profiles/screen_probe.txt; it exceeds (|x| + 2) u, which stood here before).  So e = exp(-x) errs by
// <= ((n + 4.23) A + 2) u <= ((n + 5) A + 4) u relative (|x| <= A); p = rcp(1 + e) moves by p (1 - p) <= 1/4 of that plus
// 3 u p of its own rounding: |dp| <= ((n + 5) A / 4 + 4) u + 3 u.  The +-20 clamp of the exact p adds 2.1e-9 = 2^-28.9, and
// the rounding of thr half a unit of 2^-32.  In units of 2^-16: dt <= (((n + 5) A / 4 + 7) + 2^-4.9) / 256 + 2^-17.
//   K7, five terms, n = 4: dt <= (2.25 A + 7.04) / 256 + 2^-17 < (A + 4) / 64 = the margin below, a factor >= 1.7 to spare;
//   K8, seven terms, n = 6: dt <= (2.75 A + 7.04) / 256 + 2^-17 < (4 A + 16) / 256 = the same margin, a factor >= 1.45 to
//   spare (4 / 2.75 as A grows, 16 / 7.05 at A = 0).  The comparisons themselves round h + 1 + m and h - m to fp32 (half an
//   ulp at 2^16: 1 / 256) and A, m carry a relative (n + 2) u: both far inside what is to spare ((1.25 A + 8.9) / 256).
// Non-finite A or t (huge disorder, tiny T) fail both comparisons and go to the exact branch.
// The four lines for x, A, t, m are restated in probe.hip (tsu_probe_screen), word for word: tests/test_screen_cpu.py compares the
// two texts.  A helper shared by both changed the instruction order of the sweeps, so the lines stay here as they were.
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

namespace {

// A lattice's disorder as the kernels read it: fp32 planes of rows of `pitch` elements (pad columns 0), row rho = z rows + r.
// 2-D lattices are the layer z = 0: jl, depth and pz are not read, pr = pc = periodic.
struct Geo {
    const float* jr;  // J_right, J_down, J_layer, h
    const float* jd;
    const float* jl;
    const float* h;
    long long pitch;
    int depth, rows, cols;
    int pz, pr, pc;   // periodic flag per axis
};

// One lattice's spins with the temperature and the Philox streams of its sweep
struct Walker {
    int8_t* s;    // row 0 of the spin plane (Geo's pitch)
    double T;
    float c32;    // fl32(2 / T): the screen's scale
    uint32_t k0, k1, tag_hi, tag_lo;
};

// A site's couplings to its neighbours at z - 1, z + 1, r - 1, r + 1, c - 1, c + 1 (0 where one is missing), its field and the
// screen's sum of |terms|
struct Site {
    float Jb, Jf, Ju, Jd, Jl, Jr, h, a32;
};

// A walker's spins around an octet: 16 bytes of the row and of its neighbours at z -+ 1, r -+ 1 (2-D: B and F are not read)
struct Spins {
    uint4 C, B, F, U, D;
};

// Where an octet sits: 16 consecutive columns of row (z, r), the unit of one Philox block.  Nothing here depends on the colour.
// A neighbour row that is missing on an open axis wraps to a row that exists, so every load below has a valid address and none
// needs a branch; what it brings is never used (site() gives such a neighbour J = 0 and the float64 sum skips it).
template <int DIM>
struct OctetAt {
    long long row, rowb, rowf, rowu, rowd;  // element offsets of the row and of its neighbours at z -+ 1, r -+ 1
    uint32_t rho;                           // Philox counter row: z rows + r
    int q, c0, cols, cprev;                 // cprev: column c0 - 1 (left of position 0), the last column for octet 0
    bool has_bk, has_fw, has_up, has_dn, has_prev, pc;

    __device__ __forceinline__ OctetAt(const Geo& g, int z, int r, int q_) {
        const long long layer = DIM == 3 ? (long long)z * g.rows : 0;
        q = q_;
        c0 = 16 * q;
        cols = g.cols;
        pc = g.pc;
        rho = (uint32_t)(layer + r);
        row = (layer + r) * g.pitch;
        has_up = r > 0 || g.pr;
        has_dn = r + 1 < g.rows || g.pr;
        rowu = (layer + (r > 0 ? r - 1 : g.rows - 1)) * g.pitch;
        rowd = (layer + (r + 1 < g.rows ? r + 1 : 0)) * g.pitch;
        if (DIM == 3) {
            has_bk = z > 0 || g.pz;
            has_fw = z + 1 < g.depth || g.pz;
            rowb = ((long long)(z > 0 ? z - 1 : g.depth - 1) * g.rows + r) * g.pitch;
            rowf = ((long long)(z + 1 < g.depth ? z + 1 : 0) * g.rows + r) * g.pitch;
        } else {
            has_bk = has_fw = false;
            rowb = rowf = 0;
        }
        has_prev = q > 0 || g.pc;
        cprev = q > 0 ? c0 - 1 : g.cols - 1;
    }

    // a walker's five spin vectors (the three edge bytes are update()'s)
    __device__ __forceinline__ Spins spins(const int8_t* s) const {
        Spins v;
        v.C = *reinterpret_cast<const uint4*>(s + row + c0);
        v.B = v.F = v.C;
        if (DIM == 3) {
            v.B = *reinterpret_cast<const uint4*>(s + rowb + c0);
            v.F = *reinterpret_cast<const uint4*>(s + rowf + c0);
        }
        v.U = *reinterpret_cast<const uint4*>(s + rowu + c0);
        v.D = *reinterpret_cast<const uint4*>(s + rowd + c0);
        return v;
    }
};

// One colour of an octet: its 8 sites sit at chunk positions PAR, PAR + 2, ..  Two levels, so that the single-lattice kernels keep
// their registers: rows() loads the octet's coupling rows, site(m) extracts one site from them, and update()
// takes one walker's decisions from whatever hands it the sites: site(m) itself, inside the loop (single lattices), or 8 sites
// staged once ahead of a loop over walkers (octet_group).
template <int DIM, int PAR>
struct Octet : OctetAt<DIM> {
    using At = OctetAt<DIM>;
    using At::row; using At::rowb; using At::rowu; using At::rho; using At::q; using At::c0; using At::cols; using At::cprev;
    using At::has_bk; using At::has_fw; using At::has_up; using At::has_dn; using At::has_prev; using At::pc;
    float4 jr[4], jd[4], jl[4], ju[4], jb[4], hh[4];
    float j_prev;

    __device__ __forceinline__ explicit Octet(const At& at) : At(at) {}

    // the octet's coupling rows.  A step of its own, behind every offset: at the head of a constructor, J_right's loads were hoisted
    // above the branch on the parity and waited for there before any other load was issued (3.5 % of k7_sweep and k8_sweep)
    __device__ __forceinline__ void rows(const Geo& g) {
        load16f(g.jr + row + c0, jr);
        load16f(g.jd + row + c0, jd);
        if (DIM == 3) load16f(g.jl + row + c0, jl);
        load16f(g.h + row + c0, hh);
        load16f(g.jd + rowu + c0, ju);
        if (DIM == 3) load16f(g.jl + rowb + c0, jb);
        j_prev = g.jr[row + cprev];
    }

    __device__ __forceinline__ bool has_left(int i) const { return i > 0 || has_prev; }
    __device__ __forceinline__ bool has_right(int c) const { return c + 1 < cols || pc; }

    // site m of the colour: the only place that knows how a site's couplings are read
    __device__ __forceinline__ Site site(int m) const {
        const int i = 2 * m + PAR;
        Site t;
        t.Jb = DIM == 3 && has_bk ? fat(jb, i) : 0.0f;
        t.Jf = DIM == 3 && has_fw ? fat(jl, i) : 0.0f;
        t.Ju = has_up ? fat(ju, i) : 0.0f;
        t.Jd = has_dn ? fat(jd, i) : 0.0f;
        t.Jl = has_left(i) ? (i > 0 ? fat(jr, i - 1) : j_prev) : 0.0f;
        t.Jr = has_right(c0 + i) ? fat(jr, i) : 0.0f;
        t.h = fat(hh, i);
        float a = fabsf(t.Ju);
        if (DIM == 3) a = (fabsf(t.Jb) + fabsf(t.Jf)) + a;
        t.a32 = (((a + fabsf(t.Jd)) + fabsf(t.Jl)) + fabsf(t.Jr)) + fabsf(t.h);
        return t;
    }

    // The colour's half-sweep of this octet for one walker, in place: one 16-byte store, the other colour's and the pad bytes written
    // back as read.  site_fn(m) gives site m's Site.
    template <class SiteFn>
    __device__ __forceinline__ void update(const Walker& w, uint32_t hs, const Spins& v, SiteFn site_fn) const {
        const uint4 C = v.C, B = v.B, F = v.F, U = v.U, D = v.D;
        // column c0 - 1 (left of position 0), column c0 + 16 (right of position 15, if the row has it), column 0 (right of the last
        // column, periodic)
        const int s_prev = (int)w.s[row + cprev];
        const int s_next = (c0 + 16 < cols) ? (int)w.s[row + c0 + 16] : 0;
        const int s_first = (int)w.s[row];
        const u32x4 hv = tsu_philox((uint32_t)q, rho, hs, w.tag_hi, w.k0, w.k1);
        const uint32_t wv[4] = {hv.x, hv.y, hv.z, hv.w};
        bool have_lo = false;
        uint32_t lv[4] = {0, 0, 0, 0};
        uint32_t out[4] = {C.x, C.y, C.z, C.w};
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int i = 2 * m + PAR, c = c0 + i;
            if (c >= cols) break;
            const Site t = site_fn(m);
            const int sb = sbyte(B, i), sf = sbyte(F, i), su = sbyte(U, i), sd = sbyte(D, i);
            const int sl = i > 0 ? sbyte(C, i - 1) : s_prev;
            const int sr = c + 1 < cols ? (i < 15 ? sbyte(C, i + 1) : s_next) : s_first;
            // missing neighbours carry J = 0 here: exact in fp32, and the screen only needs a bound
            float f32 = t.Ju * (float)su;
            if (DIM == 3) f32 = (t.Jb * (float)sb + t.Jf * (float)sf) + f32;
            f32 = (((f32 + t.Jd * (float)sd) + t.Jl * (float)sl) + t.Jr * (float)sr) + t.h;
            const uint32_t hi = ((wv[m >> 1] >> (16 * (m & 1))) & 0xFFFFu) ^ 0x8000u;
            int dec = screen(f32, t.a32, w.c32, hi);
            if (dec == 0) {
                // the contract's sum: neighbours in the order z-1, z+1, r-1, r+1, c-1, c+1, a missing one skipped, then h.  It starts
                // from -0.0, the identity of IEEE addition (-0.0 + x is x for every x, -0.0 included): no +0.0 enters the sum
                double f = -0.0;
                if (DIM == 3 && has_bk) f += (double)t.Jb * sb;
                if (DIM == 3 && has_fw) f += (double)t.Jf * sf;
                if (has_up) f += (double)t.Ju * su;
                if (has_dn) f += (double)t.Jd * sd;
                if (has_left(i)) f += (double)t.Jl * sl;
                if (has_right(c)) f += (double)t.Jr * sr;
                f += (double)t.h;
                const uint64_t thr = exact_thr(f, w.T);
                const uint32_t thi = (uint32_t)(thr >> 16);
                bool accept = hi < thi;
                if (hi == thi) {  // tie on the top 16 bits: the low half, as K1 draws it
                    if (!have_lo) {
                        const u32x4 l = tsu_philox((uint32_t)q, rho, hs, w.tag_lo, w.k0, w.k1);
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
        *reinterpret_cast<uint4*>(w.s + row + c0) = make_uint4(out[0], out[1], out[2], out[3]);
    }
};

// What a sweep of W walkers per lane takes: the one disorder, the walkers' tables and the walker group of the grid's z dimension.
// Ladders, ensembles and populations fill it (ladder_params); nrows and lshift are K8's lane mapping (K7: not read).
struct PTParams {
    Geo g;
    int8_t* const* s;     // walker g = ladder * R + w -> row 0 of its spin plane (one pitch for all)
    const uint32_t* key;  // walker -> Philox key (k0, k1) of seed + g
    const int32_t* slot;  // walker -> its slot in its ladder
    const double* T;      // slot -> T
    const float* c32;     // slot -> fl32(2 / T)
    int nw, W;            // walkers; walkers per lane (group z of the grid: walkers [z W, z W + W))
    uint32_t hs;
    long long nrows;      // depth * rows
    int lshift;           // log2 of the lanes per row
};

// the tables of any handle with d_s, d_key, d_slot, d_T, d_c32 (a ladder, an ensemble, a population) on the disorder g
template <class H>
PTParams ladder_params(const H* P, const Geo& g, int nw, int W) {
    PTParams p = {};
    p.g = g;
    p.s = P->d_s;
    p.key = P->d_key;
    p.slot = P->d_slot;
    p.T = P->d_T;
    p.c32 = P->d_c32;
    p.nw = nw;
    p.W = W;
    return p;
}

// One colour of the octet (z, r, q) of a single lattice: the sites are extracted as the loop comes to them
template <int DIM, int PAR>
__device__ __forceinline__ void octet_one(const Geo& g, const Walker& w, uint32_t hs, const OctetAt<DIM>& at, const Spins& v) {
    Octet<DIM, PAR> o(at);
    o.rows(g);
    o.update(w, hs, v, [&o](int m) { return o.site(m); });
}

template <int DIM>
__device__ __forceinline__ void octet_single(const Geo& g, const Walker& w, uint32_t hs, int z, int r, int q, int colour) {
    // the spin vectors go out ahead of the branch on the parity and of the rows: k8_sweep, at 4 waves per SIMD, loses 1.5 % with
    // them behind the 24 row loads
    const OctetAt<DIM> at(g, z, r, q);
    const Spins v = at.spins(w.s);
    if (((z + r + colour) & 1) == 0) octet_one<DIM, 0>(g, w, hs, at, v);
    else octet_one<DIM, 1>(g, w, hs, at, v);
}

// The same for the walkers [g0, g1): the colour's 8 sites are staged once, then each walker takes the single lattice's decision at
// the temperature of its slot, with its own key (replica 0)
template <int DIM, int PAR>
__device__ __forceinline__ void octet_walkers(const PTParams& p, int z, int r, int q, int g0, int g1) {
    Octet<DIM, PAR> o(OctetAt<DIM>(p.g, z, r, q));
    o.rows(p.g);
    Site st[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) st[m] = o.site(m);
#pragma unroll 1
    for (int g = g0; g < g1; ++g) {
        const int slot = p.slot[g];
        const Walker w = {p.s[g], p.T[slot], p.c32[slot], p.key[2 * g], p.key[2 * g + 1], TSU_TAG_ISING_HI, TSU_TAG_ISING_LO};
        o.update(w, p.hs, o.spins(w.s), [&st](int m) { return st[m]; });
    }
}

template <int DIM>
__device__ __forceinline__ void octet_group(const PTParams& p, int z, int r, int q, int g0, int g1, int colour) {
    if (((z + r + colour) & 1) == 0) octet_walkers<DIM, 0>(p, z, r, q, g0, g1);
    else octet_walkers<DIM, 1>(p, z, r, q, g0, g1);
}

// The ensemble's sample index: grid z of the sweep = sample * groups + walker group, walkers [base + group W, ..) clipped to the
// sample's own [base, base + nper), base = sample * nper; the sample's disorder sits dstride floats after its predecessor's
struct PTEns {
    long long dstride;  // floats of a sample's disorder (3 planes in 2-D, 4 in 3-D)
    int nper;           // walkers of a sample (nl * R)
    int groups;         // walker groups of a sample: ceil(nper / W)
};

// the walkers [g0, g1) of workgroup z of an ensemble's sweep, on their sample's disorder (wave-uniform)
__device__ __forceinline__ void pte_sample(Geo& g, const PTEns& e, int sample) {
    const long long off = (long long)sample * e.dstride;
    g.jr += off;
    g.jd += off;
    if (g.jl) g.jl += off;  // 2-D: no J_layer
    g.h += off;
}

__device__ __forceinline__ void pte_group(PTParams& p, const PTEns& e, int& g0, int& g1) {
    const int sample = blockIdx.z / e.groups, group = blockIdx.z - sample * e.groups;
    const int base = sample * e.nper;
    g0 = base + group * p.W;
    g1 = min(g0 + p.W, base + e.nper);
    pte_sample(p.g, e, sample);
}

// E partial of a lane: lane = chunk (rho, q), grid-stride over blockIdx.x in a fixed order; a site adds
// s (((h + J_right s_right) + J_down s_down) + J_layer s_layer), a bond missing on an open axis skipped; ssum = the lane's sum of
// spins.  Shared by the single-lattice and the ladder kernels of both dimensions: the lane order is part of the contract.
template <int DIM>
__device__ __forceinline__ double energy_lane(const Geo& g, const int8_t* s, long long& ssum) {
    const int nchunks = (g.cols + 15) >> 4;
    const long long total = (DIM == 3 ? (long long)g.depth * g.rows : (long long)g.rows) * nchunks;
    double e = 0.0;
    long long m = 0;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long rho = t / nchunks;
        const int q = (int)(t - rho * nchunks);
        const int z = DIM == 3 ? (int)(rho / g.rows) : 0, r = (int)(rho - (long long)z * g.rows);
        const long long row = rho * g.pitch;
        const bool has_dn = r + 1 < g.rows || g.pr, has_fw = DIM == 3 && (z + 1 < g.depth || g.pz);
        const long long rowd = ((long long)z * g.rows + (r + 1 < g.rows ? r + 1 : 0)) * g.pitch;
        const long long rowf = DIM == 3 ? ((long long)(z + 1 < g.depth ? z + 1 : 0) * g.rows + r) * g.pitch : 0;
        for (int i = 0; i < 16; ++i) {
            const int c = 16 * q + i;
            if (c >= g.cols) break;
            const int sc = s[row + c];
            double l = (double)g.h[row + c];
            if (c + 1 < g.cols || g.pc) l += (double)g.jr[row + c] * s[row + (c + 1 < g.cols ? c + 1 : 0)];
            if (has_dn) l += (double)g.jd[row + c] * s[rowd + c];
            if (has_fw) l += (double)g.jl[row + c] * s[rowf + c];
            e += sc * l;
            m += sc;
        }
    }
    ssum = m;
    return e;
}

}  // namespace

// potts_dev.h -- the heat-bath decision rule of the q-state Potts lattice (K10, potts_kern_dev.h and potts_host.h), written once for
// the device and for the host and once for NB = 4 neighbours (the square lattice) or 6 (the cubic one): the kernels call it, and so do
// the stand-alone host programs of the tests (tests/host/potts_rule_check.cpp, potts3d_rule_check.cpp), which is why this file
// includes nothing of HIP when a host compiler reads it.  The contract:
//   tables  E[n] = exp(J n / T), n = 0 .. NB, and F[c] = exp(h_c / T), float64, made on the host (potts_tables)
//   weights w_c = E[n_c] F[c], one rounded multiply; n_c = the neighbours that show colour c (a missing neighbour counts nowhere)
//   sums    Z_0 = w_0, Z_c = Z_{c-1} + w_c in colour order, one rounded add each
//   colour  the smallest c with (double)u Z_{q-1} < Z_c 2^32 (q - 1 if there is none), u the site's 32-bit uniform
// The multiply and the add must not fuse: on the device they are __dmul_rn / __dadd_rn, which the compiler never contracts; on the
// host contraction is switched off for the functions below (a pragma for clang, an attribute for GCC).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define POTTS_HD __host__ __device__ __forceinline__
#else
#define POTTS_HD inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define POTTS_MUL(a, b) __dmul_rn((a), (b))
#define POTTS_ADD(a, b) __dadd_rn((a), (b))
#define POTTS_NO_CONTRACT
#define POTTS_NO_CONTRACT_ATTR
#elif defined(__clang__)
#define POTTS_MUL(a, b) ((a) * (b))
#define POTTS_ADD(a, b) ((a) + (b))
#define POTTS_NO_CONTRACT _Pragma("clang fp contract(off)")
#define POTTS_NO_CONTRACT_ATTR
#else
#define POTTS_MUL(a, b) ((a) * (b))
#define POTTS_ADD(a, b) ((a) + (b))
#define POTTS_NO_CONTRACT
#define POTTS_NO_CONTRACT_ATTR __attribute__((optimize("fp-contract=off")))
#endif

#define TSU_POTTS_MAX_Q 8

template <int NB>
struct PottsTabN {
    double E[NB + 1];           // exp(J n / T)
    double F[TSU_POTTS_MAX_Q];  // exp(h_c / T); entries at c >= q are not read
    int q;
};
using PottsTab = PottsTabN<4>;   // the square lattice: E[0 .. 4]
using PottsTab6 = PottsTabN<6>;  // the cubic lattice: E[0 .. 6]

// E[n] over constant indices: no indexed load of the table (a kernel argument on the device).  The chain is written out for each
// NB because the device compiler turns this form into a branch tree over n.  The same chain from a compile-time recursion
// (n == K ? E[K] : next<K + 1>) kept every register count but compiled to NB selects a colour, which cost the 3-D heat bath 2 - 4 %
// at q = 8 (profiles/potts_shared_ab.txt, first stage); a counting loop cost the one-workgroup kernels 4 VGPRs
template <int NB>
POTTS_HD double potts_e(const PottsTabN<NB>& t, int n) {
    const double* E = t.E;
    if constexpr (NB == 4) return n == 0 ? E[0] : (n == 1 ? E[1] : (n == 2 ? E[2] : (n == 3 ? E[3] : E[4])));
    else return n == 0 ? E[0] : (n == 1 ? E[1] : (n == 2 ? E[2] : (n == 3 ? E[3] : (n == 4 ? E[4] : (n == 5 ? E[5] : E[6])))));
}

// Z_0 .. Z_7 of a site whose neighbours show the colours nb[0 .. NB - 1] (-1: no such neighbour); Z_c = Z_{q-1} for c >= q.  The
// loops run over all 8 colours and all neighbours with constant indices so that Z and nb stay in registers on the device
template <int NB>
POTTS_NO_CONTRACT_ATTR POTTS_HD void potts_cum(const PottsTabN<NB>& t, const int (&nb)[NB], double* Z) {
    POTTS_NO_CONTRACT
    double acc = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < TSU_POTTS_MAX_Q; ++c) {
        if (c < t.q) {
            int n = nb[0] == c;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int k = 1; k < NB; ++k) n += nb[k] == c;
            const double w = POTTS_MUL(potts_e(t, n), t.F[c]);
            acc = c == 0 ? w : POTTS_ADD(acc, w);
        }
        Z[c] = acc;
    }
}

// the colour for the uniform u: (double)u is exact, the product with Z_{q-1} rounds once, Z_c 2^32 is exact (a power of two)
POTTS_NO_CONTRACT_ATTR POTTS_HD int potts_pick(const double* Z, int q, uint32_t u) {
    POTTS_NO_CONTRACT
    const double lhs = POTTS_MUL((double)u, Z[TSU_POTTS_MAX_Q - 1]);
    int colour = q - 1;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = TSU_POTTS_MAX_Q - 2; c >= 0; --c)
        if (c < q - 1 && lhs < POTTS_MUL(Z[c], 4294967296.0)) colour = c;  // Z never falls, so the last hit is the smallest c
    return colour;
}

// Host only.  Step 1 of the rule, and the refusals that keep every weight finite and positive without a clamp; the bound is the
// NB-neighbour one whatever the extents of the lattice.  0: fine; else the reason
template <int NB>
inline const char* potts_tables(int q, double J, const double* h, double T, PottsTabN<NB>* t) {
    static_assert(NB == 4 || NB == 6, "the square or the cubic lattice");
    if (q < 2 || q > TSU_POTTS_MAX_Q) return "q must be in 2 .. 8";
    if (!isfinite(J)) return "J must be finite";
    if (!isfinite(T)) return "T must be finite";
    if (!(T > 0.0)) return "Temperature must be positive";
    double hmin = 0.0, hmax = 0.0;
    for (int c = 0; c < q; ++c) {
        const double v = h ? h[c] : 0.0;
        if (!isfinite(v)) return "h must be finite";
        hmin = c == 0 || v < hmin ? v : hmin;
        hmax = c == 0 || v > hmax ? v : hmax;
    }
    if (((double)NB * fabs(J) + hmax - hmin) / T > 600.0)
        return NB == 4 ? "(4 |J| + max h - min h) / T exceeds 600" : "(6 |J| + max h - min h) / T exceeds 600";
    PottsTabN<NB> tab;
    tab.q = q;
    for (int n = 0; n <= NB; ++n) tab.E[n] = exp(J * (double)n / T);
    for (int c = 0; c < TSU_POTTS_MAX_Q; ++c) tab.F[c] = c < q ? exp((h ? h[c] : 0.0) / T) : 0.0;
    // the bound above is on differences; a common offset of h can still carry exp(h_c / T) out of range
    // (the sums of 8 weights and their products with 2^32 must stay finite, the smallest weight normal)
    const double elo = tab.E[NB] < tab.E[0] ? tab.E[NB] : tab.E[0], ehi = tab.E[NB] < tab.E[0] ? tab.E[0] : tab.E[NB];
    for (int c = 0; c < q; ++c)
        if (!(elo * tab.F[c] > 1e-290) || !(ehi * tab.F[c] < 1e290)) return "exp(h_c / T) leaves the float64 range (shift h by a constant)";
    if (t) *t = tab;
    return 0;
}

// The spellings of the stand-alone host programs (tests/host/potts_rule_check.cpp, potts3d_rule_check.cpp): the neighbours one by
// one, and the six-neighbour names.  Thin forwards; the kernels and the library call the templates above
inline void potts_cum(const PottsTab& t, int up, int dn, int lf, int rt, double* Z) {
    const int nb[4] = {up, dn, lf, rt};
    potts_cum(t, nb, Z);
}

inline void potts_cum6(const PottsTab6& t, int zm, int zp, int up, int dn, int lf, int rt, double* Z) {
    const int nb[6] = {zm, zp, up, dn, lf, rt};
    potts_cum(t, nb, Z);
}

inline const char* potts_tables6(int q, double J, const double* h, double T, PottsTab6* t) { return potts_tables(q, J, h, T, t); }

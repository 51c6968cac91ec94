// potts_dev.h -- the heat-bath decision rule of the q-state Potts lattice (K10, potts2d.hip and potts3d.hip), written once for the
// device and for the host: the kernels call it, and so do the stand-alone host programs of the tests (tests/host/potts_rule_check.cpp,
// potts3d_rule_check.cpp), which is why this file includes nothing of HIP when a host compiler reads it.  The four-neighbour rule of
// the square lattice comes first, the six-neighbour one of the cubic lattice after it.  The contract:
//   tables  E[n] = exp(J n / T), n = 0 .. 4, and F[c] = exp(h_c / T), float64, made on the host (potts_tables)
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

struct PottsTab {
    double E[5];                // exp(J n / T)
    double F[TSU_POTTS_MAX_Q];  // exp(h_c / T); entries at c >= q are not read
    int q;
};

// Z_0 .. Z_7 of a site whose neighbours show the colours up, dn, lf, rt (-1: no such neighbour); Z_c = Z_{q-1} for c >= q.  The
// loops run over all 8 colours with constant indices so that Z stays in registers on the device
POTTS_NO_CONTRACT_ATTR POTTS_HD void potts_cum(const PottsTab& t, int up, int dn, int lf, int rt, double* Z) {
    POTTS_NO_CONTRACT
    double acc = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < TSU_POTTS_MAX_Q; ++c) {
        if (c < t.q) {
            const int n = (up == c) + (dn == c) + (lf == c) + (rt == c);
            const double e = n == 0 ? t.E[0] : (n == 1 ? t.E[1] : (n == 2 ? t.E[2] : (n == 3 ? t.E[3] : t.E[4])));
            const double w = POTTS_MUL(e, t.F[c]);
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

// Host only.  Step 1 of the rule, and the refusals that keep every weight finite and positive without a clamp.  0: fine; else the reason
inline const char* potts_tables(int q, double J, const double* h, double T, PottsTab* t) {
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
    if ((4.0 * fabs(J) + hmax - hmin) / T > 600.0) return "(4 |J| + max h - min h) / T exceeds 600";
    PottsTab tab;
    tab.q = q;
    for (int n = 0; n < 5; ++n) tab.E[n] = exp(J * (double)n / T);
    for (int c = 0; c < TSU_POTTS_MAX_Q; ++c) tab.F[c] = c < q ? exp((h ? h[c] : 0.0) / T) : 0.0;
    // the bound above is on differences; a common offset of h can still carry exp(h_c / T) out of range
    // (the sums of 8 weights and their products with 2^32 must stay finite, the smallest weight normal)
    const double elo = tab.E[4] < tab.E[0] ? tab.E[4] : tab.E[0], ehi = tab.E[4] < tab.E[0] ? tab.E[0] : tab.E[4];
    for (int c = 0; c < q; ++c)
        if (!(elo * tab.F[c] > 1e-290) || !(ehi * tab.F[c] < 1e290)) return "exp(h_c / T) leaves the float64 range (shift h by a constant)";
    if (t) *t = tab;
    return 0;
}

// ---------------------------------------------------------------- six neighbours (K10 in 3-D, potts3d.hip)
// The same rule on the cubic lattice: n_c runs to 6, so the table holds E[0 .. 6]; the sums and the pick are the ones above.  A
// struct and functions of their own, beside the four-neighbour ones, whose signatures and code the 2-D kernels and
// tests/host/potts_rule_check.cpp keep as they are.
struct PottsTab6 {
    double E[7];                // exp(J n / T)
    double F[TSU_POTTS_MAX_Q];  // exp(h_c / T); entries at c >= q are not read
    int q;
};

// Z_0 .. Z_7 of a site whose neighbours show the colours zm, zp (the layers below and above), up, dn, lf, rt (-1: none)
POTTS_NO_CONTRACT_ATTR POTTS_HD void potts_cum6(const PottsTab6& t, int zm, int zp, int up, int dn, int lf, int rt, double* Z) {
    POTTS_NO_CONTRACT
    double acc = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < TSU_POTTS_MAX_Q; ++c) {
        if (c < t.q) {
            const int n = (zm == c) + (zp == c) + (up == c) + (dn == c) + (lf == c) + (rt == c);
            const double e = n == 0 ? t.E[0] : (n == 1 ? t.E[1] : (n == 2 ? t.E[2] : (n == 3 ? t.E[3] : (n == 4 ? t.E[4] : (n == 5 ? t.E[5] : t.E[6])))));
            const double w = POTTS_MUL(e, t.F[c]);
            acc = c == 0 ? w : POTTS_ADD(acc, w);
        }
        Z[c] = acc;
    }
}

// Host only: potts_tables with the six-neighbour bound, whatever the depth of the lattice
inline const char* potts_tables6(int q, double J, const double* h, double T, PottsTab6* t) {
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
    if ((6.0 * fabs(J) + hmax - hmin) / T > 600.0) return "(6 |J| + max h - min h) / T exceeds 600";
    PottsTab6 tab;
    tab.q = q;
    for (int n = 0; n < 7; ++n) tab.E[n] = exp(J * (double)n / T);
    for (int c = 0; c < TSU_POTTS_MAX_Q; ++c) tab.F[c] = c < q ? exp((h ? h[c] : 0.0) / T) : 0.0;
    const double elo = tab.E[6] < tab.E[0] ? tab.E[6] : tab.E[0], ehi = tab.E[6] < tab.E[0] ? tab.E[0] : tab.E[6];
    for (int c = 0; c < q; ++c)
        if (!(elo * tab.F[c] > 1e-290) || !(ehi * tab.F[c] < 1e290)) return "exp(h_c / T) leaves the float64 range (shift h by a constant)";
    if (t) *t = tab;
    return 0;
}

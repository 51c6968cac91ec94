// potts_disorder_dev.h -- the heat-bath decision rule of the q-state Potts lattice with per-bond couplings and per-site colour fields
// (K12, potts_disorder_kern_dev.h and potts_disorder.hip), written once for the device and for the host, in the manner of potts_dev.h
// (whose macros it uses): the kernels call it, tsu_potts_dis_site_thresholds calls it, and so does the stand-alone host program of the
// tests (tests/host/potts_disorder_rule_check.cpp).  It includes nothing of HIP when a host compiler reads it.  The contract
// (DESIGN.md section 3), for a site with the existing neighbours k in the order z-1, z+1, r-1, r+1, c-1, c+1:
//   sums     a_c = (double)h[c] (0.0 without a field), then + (double)J_k for every neighbour k, in that order, that shows colour c:
//            one rounded add each; a neighbour that does not show c adds nothing
//   weights  a* = max_c a_c, x_c = (a_c - a*) / T (one rounded subtract, one correctly rounded divide), w_c = exp(x_c): w = 1 at
//            the maximum, nothing overflows, an underflow to 0 is harmless
//   sums     Z_0 = w_0, Z_c = Z_{c-1} + w_c in colour order, one rounded add each
//   colour   thr_c = (uint64)floor(Z_c / Z_{q-1} 2^32 + 0.5) for c < q - 1, thr_{q-1} = 2^32; the smallest c with (uint64)u < thr_c
// The thresholds are integers, so an ulp between the device's exp and the C library's moves a decision only when u equals a
// threshold that the ulp moved (tests/helpers/potts_disorder_twin.py, fragile).  The pick is monotone in u.
#pragma once
#include "potts_dev.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define PD_SUB(a, b) __dsub_rn((a), (b))
#define PD_DIV(a, b) __ddiv_rn((a), (b))
#define PD_UNROLL _Pragma("unroll")
#else
#define PD_SUB(a, b) ((a) - (b))
#define PD_DIV(a, b) ((a) / (b))
#define PD_UNROLL
#endif

// Steps 2 - 5 for the sums a[0 .. q - 1]: thr[c] for all 8 colours (2^32 from q - 1 on).  The loops run over all 8 colours with
// constant indices so that a, Z and thr stay in registers on the device
POTTS_NO_CONTRACT_ATTR POTTS_HD void pd_thresholds(int q, const double (&a)[TSU_POTTS_MAX_Q], double T, uint64_t (&thr)[TSU_POTTS_MAX_Q]) {
    POTTS_NO_CONTRACT
    double amax = a[0];
    PD_UNROLL
    for (int c = 1; c < TSU_POTTS_MAX_Q; ++c)
        if (c < q && a[c] > amax) amax = a[c];
    double Z[TSU_POTTS_MAX_Q];
    double acc = 0.0;
    PD_UNROLL
    for (int c = 0; c < TSU_POTTS_MAX_Q; ++c) {
        if (c < q) {
            const double w = exp(PD_DIV(PD_SUB(a[c], amax), T));
            acc = c == 0 ? w : POTTS_ADD(acc, w);
        }
        Z[c] = acc;
    }
    PD_UNROLL
    for (int c = 0; c < TSU_POTTS_MAX_Q; ++c) {
        const double t = POTTS_ADD(POTTS_MUL(PD_DIV(Z[c], acc), 4294967296.0), 0.5);  // the product is exact (a power of two)
        thr[c] = c < q - 1 ? (uint64_t)floor(t) : 4294967296ull;
    }
}

// Step 1 and the rest for one site: nb[k] the colour of neighbour k (-1: no such neighbour), J[k] its coupling, hv[c] the field
// (not read without one)
template <int NB, bool HAS_H>
POTTS_NO_CONTRACT_ATTR POTTS_HD void pd_site_thresholds(int q, double T, const int (&nb)[NB], const float (&J)[NB],
                                                        const float (&hv)[TSU_POTTS_MAX_Q], uint64_t (&thr)[TSU_POTTS_MAX_Q]) {
    POTTS_NO_CONTRACT
    double a[TSU_POTTS_MAX_Q];
    PD_UNROLL
    for (int c = 0; c < TSU_POTTS_MAX_Q; ++c) {
        double v = 0.0;
        if (c < q) {
            if (HAS_H) v = (double)hv[c];
            PD_UNROLL
            for (int k = 0; k < NB; ++k)
                if (nb[k] == c) v = POTTS_ADD(v, (double)J[k]);
        }
        a[c] = v;
    }
    pd_thresholds(q, a, T, thr);
}

// the smallest c with u < thr[c]; thr[q - 1] = 2^32 ends the search
POTTS_HD int pd_pick(const uint64_t (&thr)[TSU_POTTS_MAX_Q], uint32_t u) {
    int colour = TSU_POTTS_MAX_Q - 1;
    PD_UNROLL
    for (int c = TSU_POTTS_MAX_Q - 2; c >= 0; --c)
        if ((uint64_t)u < thr[c]) colour = c;  // thr never falls, so the last hit is the smallest c
    return colour;
}

// the threshold of a bond of coupling J >= 0 between two equal colours (Swendsen-Wang steps): floor(-expm1(-J / T) 2^32); J = 0, a
// diluted bond, gives 0 and is never active
POTTS_HD uint64_t pd_bond_threshold(float J, double T) {
    const double p = -expm1(PD_DIV(-(double)J, T));
    return (uint64_t)floor(p * 4294967296.0);
}

// potts_disorder_rule_check.cpp -- the heat-bath rule of csrc/potts_disorder_dev.h (the header K12's kernels use) evaluated on the
// host, for tests/test_potts_disorder_cpu.py: the test compiles this file with the host compiler, feeds it one record per site and
// compares the thresholds and the colours with the NumPy twin.  Compiled with the target's fused multiply-add enabled, so an
// operation that contracts would show as a different threshold.
//
// usage: potts_disorder_rule_check q T has_h < records > lines
//   a record is 6 signed bytes (the neighbours' colours in the order z-1, z+1, r-1, r+1, c-1, c+1; -1: none), 2 pad bytes, 6 floats
//   (their couplings), 8 floats (the site's field per colour) and a little-endian uint32 u: 68 bytes in all
//   output: one line per record, the colour and then thr_0 .. thr_{q-1}
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "potts_disorder_dev.h"

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const int q = atoi(argv[1]), has_h = atoi(argv[3]);
    const double T = strtod(argv[2], nullptr);
    if (q < 2 || q > TSU_POTTS_MAX_Q || !(T > 0.0)) return 2;
    unsigned char rec[68];
    while (fread(rec, 1, sizeof(rec), stdin) == sizeof(rec)) {
        int8_t b[6];
        int nb[6];
        float J[6], hv[TSU_POTTS_MAX_Q];
        uint32_t u;
        memcpy(b, rec, 6);
        memcpy(J, rec + 8, 24);
        memcpy(hv, rec + 32, 32);
        memcpy(&u, rec + 64, 4);
        for (int k = 0; k < 6; ++k) nb[k] = b[k];
        uint64_t thr[TSU_POTTS_MAX_Q];
        if (has_h) pd_site_thresholds<6, true>(q, T, nb, J, hv, thr);
        else pd_site_thresholds<6, false>(q, T, nb, J, hv, thr);
        printf("%d", pd_pick(thr, u));
        for (int c = 0; c < q; ++c) printf(" %llu", (unsigned long long)thr[c]);
        printf("\n");
    }
    return 0;
}

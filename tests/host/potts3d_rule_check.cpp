// potts3d_rule_check.cpp -- the six-neighbour Potts heat-bath rule of csrc/potts_dev.h (the header the 3-D kernels use) evaluated on
// the host, for tests/test_potts3d_cpu.py: the test compiles this file with the host compiler, feeds it (zm, zp, up, dn, lf, rt, u)
// records and compares the colours with the NumPy twin.  Compiled with the target's fused multiply-add enabled, so a product and a
// sum that contract would show as a different colour on the near-tie inputs.
//
// usage: potts3d_rule_check q J T h_0 .. h_{q-1} < records > colours
//   a record is 6 signed bytes (the neighbours' colours, -1: none), 2 pad bytes and a little-endian uint32 u, 12 bytes in all
//   output: the 15 table values as hexadecimal floats on the first line, then one colour per line
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "potts_dev.h"

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const int q = atoi(argv[1]);
    const double J = strtod(argv[2], nullptr), T = strtod(argv[3], nullptr);
    if (q < 2 || q > TSU_POTTS_MAX_Q || argc != 4 + q) return 2;
    double h[TSU_POTTS_MAX_Q] = {};
    for (int c = 0; c < q; ++c) h[c] = strtod(argv[4 + c], nullptr);
    PottsTab6 tab;
    const char* why = potts_tables6(q, J, h, T, &tab);
    if (why) {
        fprintf(stderr, "refused: %s\n", why);
        return 3;
    }
    for (int n = 0; n < 7; ++n) printf("%a ", tab.E[n]);
    for (int c = 0; c < TSU_POTTS_MAX_Q; ++c) printf("%a%c", tab.F[c], c + 1 < TSU_POTTS_MAX_Q ? ' ' : '\n');
    unsigned char rec[12];
    while (fread(rec, 1, 12, stdin) == 12) {
        int8_t nb[6];
        uint32_t u;
        memcpy(nb, rec, 6);
        memcpy(&u, rec + 8, 4);
        double Z[TSU_POTTS_MAX_Q];
        potts_cum6(tab, nb[0], nb[1], nb[2], nb[3], nb[4], nb[5], Z);
        printf("%d\n", potts_pick(Z, q, u));
    }
    return 0;
}

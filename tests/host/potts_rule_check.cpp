// potts_rule_check.cpp -- the Potts heat-bath rule of csrc/potts_dev.h (the header the kernels use) evaluated on the host, for
// tests/test_potts_cpu.py: the test compiles this file with the host compiler, feeds it (up, dn, lf, rt, u) records and compares the
// colours with the NumPy twin.  Compiled with the target's fused multiply-add enabled, so a product and a sum that contract would
// show as a different colour on the near-tie inputs.
//
// usage: potts_rule_check q J T h_0 .. h_{q-1} < records > colours
//   a record is 4 signed bytes (the neighbours' colours, -1: none) and a little-endian uint32 u, 8 bytes in all
//   output: the 13 table values as hexadecimal floats on the first line, then one colour per line
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
    PottsTab tab;
    const char* why = potts_tables(q, J, h, T, &tab);
    if (why) {
        fprintf(stderr, "refused: %s\n", why);
        return 3;
    }
    for (int n = 0; n < 5; ++n) printf("%a ", tab.E[n]);
    for (int c = 0; c < TSU_POTTS_MAX_Q; ++c) printf("%a%c", tab.F[c], c + 1 < TSU_POTTS_MAX_Q ? ' ' : '\n');
    unsigned char rec[8];
    while (fread(rec, 1, 8, stdin) == 8) {
        int8_t nb[4];
        uint32_t u;
        memcpy(nb, rec, 4);
        memcpy(&u, rec + 4, 4);
        double Z[TSU_POTTS_MAX_Q];
        potts_cum(tab, nb[0], nb[1], nb[2], nb[3], Z);
        printf("%d\n", potts_pick(Z, q, u));
    }
    return 0;
}

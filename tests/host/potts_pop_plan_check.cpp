// Stand-alone host program over csrc/potts_pop_plan.h, K14's packing rule (tests/test_potts_pop_cpu.py builds it with the host
// compiler, with and without -fsanitize=address,undefined, and compares its output with the Python mirror in
// tests/helpers/potts_pop_twin.py).  For every site count 1 .. 16400 it prints one line: the count and a 64-bit fold of the plans
// of all (lanes, DIM, q, field, R); then the plans of a few named shapes in full; then the invariants it checked itself.
#include <cstdint>
#include <cstdio>

#include "potts_pop_plan.h"

static uint64_t fold(uint64_t h, long long v) { return (h * 1099511628211ull) ^ (uint64_t)v; }

int main() {
    const int Rs[4] = {2, 3, 255, 65535};
    int failed = 0;
    for (long long sites = 1; sites <= 16400; ++sites) {
        uint64_t h = 1469598103934665603ull;
        const long long lane_choices[2] = {(sites + 15) / 16, sites};  // one row of `sites` columns; `sites` rows of one column
        for (long long lanes : lane_choices)
            for (int dim = 2; dim <= 3; ++dim)
                for (int q = 2; q <= 8; ++q)
                    for (int field = 0; field <= 1; ++field)
                        for (int R : Rs) {
                            const PottsPopPlan p = potts_pop_plan(sites, lanes, dim, q, field, R, 1, 1);
                            h = fold(fold(fold(fold(h, p.route), p.G), p.threads), p.lds_bytes);
                            // what the kernels rely on
                            bool ok = p.threads >= 64 && p.threads <= 1024 && p.threads % 64 == 0 && p.G >= 1 && p.G <= R;
                            if (p.route == kPopRoutePack)
                                ok = ok && p.G >= 2 && (long long)p.G * lanes <= p.threads && p.threads <= kPopPackThreads && p.lds_bytes <= kPopPackLds &&
                                     p.lds_bytes >= 4 * ((dim == 2 ? 2 : 3) + (field ? q : 0)) * sites + p.G * sites;
                            else
                                ok = ok && p.G == 1;
                            if (p.route == kPopRouteSmall) ok = ok && sites <= kPopSmallSites;
                            if (p.route == kPopRouteSweep) ok = ok && sites > kPopSmallSites;
                            // the switches: no pack without the pack switch, everything on the HBM route without the small switch
                            ok = ok && potts_pop_plan(sites, lanes, dim, q, field, R, 0, 1).route != kPopRoutePack;
                            ok = ok && potts_pop_plan(sites, lanes, dim, q, field, R, 1, 0).route == kPopRouteSweep;
                            if (!ok) {
                                ++failed;
                                printf("FAIL sites %lld lanes %lld dim %d q %d field %d R %d\n", sites, lanes, dim, q, field, R);
                            }
                        }
        printf("%lld %016llx\n", sites, (unsigned long long)h);
    }
    const long long named[][5] = {{256, 16, 2, 3, 0}, {256, 16, 2, 8, 1}, {1024, 64, 2, 8, 1}, {512, 64, 3, 8, 1}, {4096, 256, 3, 3, 0}, {192, 12, 2, 3, 1}};
    for (const auto& s : named) {
        const PottsPopPlan p = potts_pop_plan(s[0], s[1], (int)s[2], (int)s[3], (int)s[4], 70, 1, 1);
        printf("plan %lld %lld %lld %lld %lld: %d %d %d %d\n", s[0], s[1], s[2], s[3], s[4], p.route, p.G, p.threads, p.lds_bytes);
    }
    printf("%d failed\n", failed);
    return failed != 0;
}

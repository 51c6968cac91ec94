// potts_pop_plan.h -- the packing rule of K14 (potts_pop.hip): which sweep kernel a population of Potts lattices takes, how many
// walkers share a workgroup, how many lanes it has and how much LDS it declares.  A pure host function of the shape, with nothing of
// HIP in it: potts_pop.hip calls it, tsu_potts_pop_plan returns it, the stand-alone host program of the tests
// (tests/host/potts_pop_plan_check.cpp) prints it and tests/helpers/potts_pop_twin.py mirrors it.  DESIGN.md section 5, "K14", has
// the reasons for the constants.
//
//   lanes   a lane owns an octet (16 columns of one global row): lanes = depth rows ceil(cols / 16) per walker
//   _PACK   lanes <= kPopPackMaxLanes, so that G = min(kPopPackThreads / lanes, R) >= 2 walkers share a workgroup of
//           ceil64(G lanes) lanes, and the workgroup's LDS, the disorder once (4 bytes a site and plane: 2 or 3 coupling planes, q
//           field planes with a field) and G colour planes at the walkers' stride (sites rounded up to 16), is at most kPopPackLds
//   _SMALL  any other lattice of at most kPopSmallSites sites: one workgroup per walker, min(ceil64(lanes), 1024) lanes, the
//           colours in a fixed array of kPopSmallSites bytes
//   _SWEEP  the rest: 256 lanes a workgroup, no LDS
#pragma once

constexpr int kPopRoutePack = 0, kPopRouteSmall = 1, kPopRouteSweep = 2;  // TSU_POTTS_POP_ROUTE_*
constexpr int kPopPackThreads = 256;      // the launch bound of k14_pop_pack: four waves, one per SIMD, no scratch at 512 VGPRs a lane
constexpr int kPopPackMaxLanes = 128;     // G >= 2 at kPopPackThreads
constexpr int kPopPackLds = 64 * 1024;    // at least two workgroups a CU (160 KiB)
constexpr int kPopSmallSites = 16384;     // kPottsSmallSites
constexpr int kPopSmallMaxThreads = 1024; // kSwMaxThreads

struct PottsPopPlan {
    int route, G, threads, lds_bytes;
};

inline long long potts_pop_stride(long long sites) { return (sites + 15) / 16 * 16; }

// allow_pack / allow_small: the environment switches (TSU_POTTS_POP_PACK, TSU_POTTS_SMALL) as the caller read them; 1, 1 is the
// shipped rule
inline PottsPopPlan potts_pop_plan(long long sites, long long lanes, int dim, int q, int has_field, int R, int allow_pack, int allow_small) {
    PottsPopPlan p = {kPopRouteSweep, 1, 256, 0};
    if (!allow_small || sites > kPopSmallSites) return p;
    const long long t = (lanes + 63) / 64 * 64;
    p.route = kPopRouteSmall;
    p.threads = (int)(t < kPopSmallMaxThreads ? t : kPopSmallMaxThreads);
    p.lds_bytes = kPopSmallSites;
    if (!allow_pack || lanes > kPopPackMaxLanes) return p;
    const int fit = (int)(kPopPackThreads / lanes);
    const int G = fit < R ? fit : R;
    const long long planes = (dim == 2 ? 2 : 3) + (has_field ? q : 0);
    const long long lds = 4 * planes * sites + (long long)G * potts_pop_stride(sites);
    if (G < 2 || lds > kPopPackLds) return p;
    p.route = kPopRoutePack;
    p.G = G;
    p.threads = (int)(((long long)G * lanes + 63) / 64 * 64);
    p.lds_bytes = (int)lds;
    return p;
}

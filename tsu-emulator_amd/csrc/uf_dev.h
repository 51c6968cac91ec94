// uf_dev.h -- device helpers shared by the cluster kernels (K6 ising2d_cluster.hip and K8 ising3d_cluster.hip through sw_dev.h, K7
// replica cluster moves ising2d_icm.hip): one union-find with min-index roots in LDS or HBM, with or without the ghost label -1 (K8 in
// a field only), the capped-loop error flag and the one-coin-per-root rule.
#pragma once
#include "tsu_common.h"

namespace {

constexpr int kBudget = 1 << 20;  // union / find steps one lane may take per call of a union

// ---------------------------------------------------------------- union-find with min-index roots (LDS or HBM)
// GHOST: label -1 is legal.  The ghost is an index below every site, so min-index roots take it as they are: a tree linked under -1
// is frozen.  A find that loads a negative parent returns -1 and never indexes with it; a or b of a union may be -1 themselves.
// GHOST = false compiles the tests for it out.
template <int SCOPE>
__device__ __forceinline__ int uf_load(const int* L, int x) {
    return __hip_atomic_load(L + x, __ATOMIC_RELAXED, SCOPE);
}

// root of x, halving the path on the way (each halving step is an atomicMin to an ancestor: it can only shorten the path)
template <bool GHOST, int SCOPE>
__device__ __forceinline__ int uf_find(int* L, int x, int& budget) {
    if constexpr (GHOST)
        if (x < 0) return -1;
    int p = uf_load<SCOPE>(L, x);
    while (p != x) {
        if constexpr (GHOST)
            if (p < 0) return -1;
        const int gp = uf_load<SCOPE>(L, p);
        if (gp == p) return p;
        __hip_atomic_fetch_min(L + x, gp, __ATOMIC_RELAXED, SCOPE);
        if constexpr (GHOST)
            if (gp < 0) return -1;
        x = gp;
        p = uf_load<SCOPE>(L, x);
        if (--budget < 0) return x;
    }
    return x;
}

// join the trees of a and b: link the larger root under the smaller one.  If that root got a parent meanwhile, atomicMin
// returned the parent it had: join that parent with the smaller root next (nothing is lost, every index only falls).
// GHOST: joins two free trees, a free and a frozen one (b = -1 is a site's ghost bond), or two frozen ones (both roots -1: nothing
// to do).  The larger root is a site (>= 0), so the atomicMin never indexes with the ghost; if that root got a parent meanwhile
// (-1 included) the loop goes on from it.
template <bool GHOST, int SCOPE>
__device__ __forceinline__ bool uf_union(int* L, int a, int b, int& budget) {
    for (;;) {
        a = uf_find<GHOST, SCOPE>(L, a, budget);
        b = uf_find<GHOST, SCOPE>(L, b, budget);
        if (budget < 0) return false;
        if (a == b) return true;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return true;
        a = old;
        if (--budget < 0) return false;
    }
}

__device__ __forceinline__ void raise_err(int* err) {
    __hip_atomic_store(err, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ uint32_t word_of(const u32x4& w, int m) { return m == 0 ? w.x : (m == 1 ? w.y : (m == 2 ? w.z : w.w)); }

// the coin of the cluster rooted at (r, c): bit 31 of word c & 3 of Philox(c >> 2, r, t, tag)
__device__ __forceinline__ bool flip_bit(int r, int c, uint32_t t, uint32_t tag, uint32_t k0, uint32_t k1) {
    const u32x4 w = tsu_philox((uint32_t)c >> 2, (uint32_t)r, t, tag, k0, k1);
    const int m = c & 3;
    const uint32_t v = m == 0 ? w.x : (m == 1 ? w.y : (m == 2 ? w.z : w.w));
    return (v >> 31) != 0;
}

}  // namespace

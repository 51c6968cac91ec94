// sw_dev.h -- what the Swendsen-Wang kernels of K6 (ising2d_cluster.hip: DIM = 2, one J) and K8 (ising3d_cluster.hip: DIM = 3,
// per-bond J, GHOST for a field) share on the device: the geometry, key, item and parameter structs, the two bond policies, the seam
// decoder of the merge pass, the root chase and the resolve pass.  Step t of a D x R x C lattice (D = 1 at DIM = 2), global row
// rho = z R + r, site index i = rho C + c:
//   bond    right and down bonds of (rho, c): W = Philox(c >> 1, rho, t, tag_bond), right W[2 (c & 1)], down W[2 (c & 1) + 1];
//           DIM = 3: the layer bond to z + 1: word c & 3 of Philox(c >> 2, rho, t, tag_layer); GHOST: the bond to the ghost spin:
//           word c & 3 of Philox(c >> 2, rho, t, tag_ghost).  Whether a bond with word u is active is the bond policy's answer
//   labels  union-find with min-index roots (uf_dev.h); GHOST: a component joined to the ghost has root -1 and is frozen
//   flip    the cluster rooted at (rho, c) flips iff flip_bit(rho, c, t, tag_flip)
// The __global__ kernels stay in their files with their own launch bounds.  DIM = 2 compiles every z term out (no depth, no third
// seam family; rows stay ints).  The seam decoder and the root chase serve K7's replica cluster moves (ising2d_icm.hip) as well.
#pragma once
#include <type_traits>

#include "uf_dev.h"

namespace {

struct SwGeom {
    long long pitch;
    int depth, rows, cols;  // DIM = 2: depth is 1 and never read on the device
    int pz, pr, pc;         // periodic flag per axis
    int tz, tr, tc;         // tile shape (tc even: a right / down Philox block never straddles two tiles)
    int nz, nr, nc;         // tiles per axis
};

struct SwKeys {
    uint32_t k0, k1, tag_bond, tag_layer, tag_flip, tag_ghost;
    uint32_t t;  // the step; in an item: the first step of the call
};

// ---------------------------------------------------------------- bond policies: coupling(axis, g) of the bond that leaves the
// site at element g along axis 0 (right), 1 (down) or 2 (layer); sat: J s s' > 0; on: sat and u < thr(J, T)
struct SwUniformBonds {  // K6: one J, its threshold computed on the host (thr may be 2^32: 64-bit compare); no layer, no ghost
    uint64_t thr;
    int jsign;
    __device__ __forceinline__ int coupling(int, long long) const { return jsign; }
    __device__ __forceinline__ static bool sat(int J, int sa, int sb) { return J * sa * sb > 0; }
    __device__ __forceinline__ bool on(int J, int sa, int sb, uint32_t u) const { return sat(J, sa, sb) && (uint64_t)u < thr; }
};

struct SwStoredBonds {  // K8: fp32 planes; thr = floor(-expm1(-2 |J| / T) 2^32) in float64 from the stored value, per satisfied bond
    const float* jr;
    const float* jd;
    const float* jl;
    const float* h;  // read by the ghost kernels only
    double T;
    __device__ __forceinline__ float coupling(int axis, long long g) const { return (axis == 0 ? jr : (axis == 1 ? jd : jl))[g]; }
    __device__ __forceinline__ static bool sat(float J, int sa, int sb) { return ((J > 0.0f) - (J < 0.0f)) * sa * sb > 0; }
    __device__ __forceinline__ bool on(float J, int sa, int sb, uint32_t u) const {
        if (!sat(J, sa, sb)) return false;
        const double p = -expm1((-2.0 * fabs((double)J)) / T);
        return (uint64_t)u < (uint64_t)floor(p * 4294967296.0);
    }
};

template <class Bonds>
struct SwItem {  // one lattice of the one-workgroup route
    int8_t* s;   // row 0
    Bonds b;
    SwKeys k;
};

template <class Bonds>
struct SwParams {  // one step of the multi-tile route
    int8_t* s;
    Bonds b;
    int* labels;  // depth * rows * cols; -1 (GHOST only): the site's component is frozen
    SwGeom g;
    SwKeys k;
    int* err;
};

template <int DIM>
using sw_row_t = std::conditional_t<DIM == 2, int, long long>;  // a global row; K6's rows are ints

// ---------------------------------------------------------------- seams
// lanes of a merge launch: sc D R right bonds of the column seams, sr D C down bonds of the row seams, sz R C layer bonds
template <int DIM>
__host__ __device__ __forceinline__ long long sw_seam_lanes(const SwGeom& g) {
    const long long depth = DIM == 3 ? g.depth : 1;
    long long n = (g.nc - 1 + g.pc) * depth * g.rows + (g.nr - 1 + g.pr) * depth * g.cols;
    if constexpr (DIM == 3) n += (long long)(g.nz - 1 + g.pz) * g.rows * g.cols;
    return n;
}

// lane -> the bond (rho, c) - (rho2, c2) and its axis; -1 past the last lane.  Lanes [0, sc D R): seam k < nc - 1 at column
// (k + 1) tc - 1, the last one of a periodic axis at column cols - 1, wrapping to 0; then the row seams, then the layer seams
template <int DIM>
__device__ __forceinline__ int sw_seam(const SwGeom& g, long long lane, sw_row_t<DIM>& rho, int& c, sw_row_t<DIM>& rho2, int& c2) {
    using row_t = sw_row_t<DIM>;
    const int depth = DIM == 3 ? g.depth : 1;
    const long long nrows = (long long)depth * g.rows;
    const long long lc_n = (long long)(g.nc - 1 + g.pc) * nrows, lr_n = (long long)(g.nr - 1 + g.pr) * depth * g.cols;
    if (lane >= sw_seam_lanes<DIM>(g)) return -1;
    if (lane < lc_n) {
        const int k = (int)(lane / nrows);
        rho = rho2 = (row_t)(lane - (long long)k * nrows);
        c = k < g.nc - 1 ? (k + 1) * g.tc - 1 : g.cols - 1;
        c2 = c + 1 < g.cols ? c + 1 : 0;
        return 0;
    }
    if (DIM == 2 || lane < lc_n + lr_n) {
        const long long l = lane - lc_n, per = (long long)depth * g.cols;
        const int k = (int)(l / per);
        const long long rem = l - (long long)k * per;
        const int z = DIM == 3 ? (int)(rem / g.cols) : 0;
        c = c2 = (int)(rem - (long long)z * g.cols);
        const int r = k < g.nr - 1 ? (k + 1) * g.tr - 1 : g.rows - 1;
        rho = (row_t)z * g.rows + r;
        rho2 = (row_t)z * g.rows + (r + 1 < g.rows ? r + 1 : 0);
        return 1;
    }
    if constexpr (DIM == 3) {
        const long long l = lane - lc_n - lr_n, per = (long long)g.rows * g.cols;
        const int k = (int)(l / per);
        const long long rem = l - (long long)k * per;
        const int r = (int)(rem / g.cols);
        c = c2 = (int)(rem - (long long)r * g.cols);
        const int z = k < g.nz - 1 ? (k + 1) * g.tz - 1 : g.depth - 1;
        rho = (long long)z * g.rows + r;
        rho2 = (long long)(z + 1 < g.depth ? z + 1 : 0) * g.rows + r;
    }
    return 2;
}

// label x -> the root of its tree in HBM (no halving: the trees are final); GHOST: a chain that ends in -1 is frozen
template <bool GHOST>
__device__ __forceinline__ int sw_chase(const int* labels, int x, bool& bad) {
    int budget = kBudget;
    if (!GHOST || x >= 0) {
        for (int y = labels[x]; y != x; y = labels[x]) {
            x = y;
            if (GHOST && x < 0) break;
            if (--budget < 0) {
                bad = true;
                break;
            }
        }
    }
    return x;
}

// ---------------------------------------------------------------- multi-tile route: resolve
// The kernels that run a union-find (the one-workgroup kernel, the local pass of the tiles, the merge pass after its seam decoder)
// keep their bodies in their own files, on the structs and bond policies above.  A body shared through a function reads the
// kernel's parameters through a pointer; the compiler then orders the loads and the union-find loops around them differently (one
// more v_mov per path-halving step), which cost the local kernels 1.3 - 2.3 %, the one-workgroup kernels up to 1.6 % and the merge
// pass of an ordered lattice more (profiles/cluster_shared_body_time.txt).  SwParams lists the bond policy ahead of the geometry
// because k8_sw_local then fetches all its arguments in one batch (the other order cost it a second wait, 0.7 us a launch).

// One lane (of 256 a workgroup) per 4 sites of a global row (one 4-byte load and store; the pad bytes beyond cols are 0 and stay
// 0): the root of each site, the root's coin (one Philox block per distinct root of the lane), the spin rewritten in place.  GHOST:
// a frozen component draws no coin, the spin stays
template <int DIM, bool GHOST, class Bonds>
__device__ __forceinline__ void sw_resolve(const SwParams<Bonds>& p, int quads) {
    const SwGeom& g = p.g;
    const long long lane = (long long)blockIdx.x * 256 + threadIdx.x;
    const sw_row_t<DIM> rho = (sw_row_t<DIM>)(lane / quads);
    const int c0 = 4 * (int)(lane - (long long)rho * quads);
    if (rho >= (sw_row_t<DIM>)(DIM == 3 ? g.depth : 1) * g.rows) return;
    int8_t* const row = p.s + (long long)rho * g.pitch;
    uint32_t v = *reinterpret_cast<const uint32_t*>(row + c0);
    int last = -1;
    bool last_flip = false, bad = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (c0 + j >= g.cols) break;
        const int x = sw_chase<GHOST>(p.labels, p.labels[(long long)rho * g.cols + c0 + j], bad);
        if (GHOST && x < 0) {
            last = x;
            last_flip = false;
        } else if (x != last) {
            const int rr = x / g.cols, rc = x - rr * g.cols;
            last = x;
            last_flip = flip_bit(rr, rc, p.k.t, p.k.tag_flip, p.k.k0, p.k.k1);
        }
        if (last_flip) {
            const uint32_t b = (v >> (8 * j)) & 0xFFu;
            v = (v & ~(0xFFu << (8 * j))) | (((uint32_t)(-(int)(int8_t)b) & 0xFFu) << (8 * j));
        }
    }
    *reinterpret_cast<uint32_t*>(row + c0) = v;
    if (bad) raise_err(p.err);
}

}  // namespace

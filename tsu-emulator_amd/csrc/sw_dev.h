// sw_dev.h -- what the Swendsen-Wang kernels of K6 (ising2d_cluster.hip: DIM = 2, one J) and K8 (ising3d_cluster.hip: DIM = 3,
// per-bond J, GHOST for a field) share on the device: the geometry, key, item and parameter structs, the two bond policies, the seam
// decoder of the merge pass, the root chase and the resolve pass.  Step t of a D x R x C lattice (D = 1 at DIM = 2), global row
// rho = z R + r, site index i = rho C + c:
//   bond    right and down bonds of (rho, c): W = Philox(c >> 1, rho, t, tag_bond), right W[2 (c & 1)], down W[2 (c & 1) + 1];
//           DIM = 3: the layer bond to z + 1: word c & 3 of Philox(c >> 2, rho, t, tag_layer); GHOST: the bond to the ghost spin:
//           word c & 3 of Philox(c >> 2, rho, t, tag_ghost).  Whether a bond with word u is active is the bond policy's answer
//   labels  union-find with min-index roots (uf_dev.h); GHOST: a component joined to the ghost has root -1 and is frozen
//   flip    the cluster rooted at (rho, c) flips iff flip_bit(rho, c, t, tag_flip)
// The __global__ kernels of a step stay in their files with their own launch bounds (the measuring passes of the cluster-size
// records, which read no bond, are at the end of this file).  DIM = 2 compiles every z term out (no depth, no third
// seam family; rows stay ints).  The seam decoder and the root chase serve K7's replica cluster moves (ising2d_icm.hip) as well.
// K10's Potts lattices (potts_kern_dev.h, both dimensions) use the structs, the seam decoder and the root chase with a bond policy
// of their own (PottsBonds: two equal colours) and their own resolve pass, which writes a colour instead of flipping a spin.
#pragma once
#include <type_traits>

#include "uf_dev.h"

namespace {

constexpr int kSwMaxThreads = 1024;  // the launch bound of the one-workgroup kernels and of the 3-D tile pass; the host's lane cap

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

// ---------------------------------------------------------------- cluster-size records (tsu_hip_cluster_measure.h)
// One row of 8 words per step: n_clusters, largest, sum |C|^2, sum M_C^2, sum M_C^4 (low, high), n_frozen, m_frozen.  Integers only:
// packed (up, down) site counts per root, wave and workgroup reductions, integer atomics; the 128-bit sum carries by hand.  The
// unmeasured kernels carry none of this: the one-workgroup kernels have a measured instantiation with one more argument
// (SwRecOut), the multi-tile route runs three passes of its own (sw_meas_count, sw_meas_fold, sw_meas_row) on the labels the
// unmeasured kernels leave in HBM.  Those passes read no bond and draw no random word, so they are written once, here, for both
// dimensions and for the ghost (label -1) alike.

struct SwRecOut {  // the extra argument of a measured one-workgroup kernel: where workgroup b writes its rows
    long long* const* rows_of;  // a batch: row 0 of every lattice (a device array); NULL: one lattice
    long long* rows_one;
};

__device__ __forceinline__ long long* sw_rec_rows(const SwRecOut& r) { return r.rows_of ? r.rows_of[blockIdx.x] : r.rows_one; }

// the measured one-workgroup kernels' static LDS: s_row[6], then the frozen sites' (up, down) as two dwords; the plain
// instantiations declare none
template <bool MEAS>
__device__ __forceinline__ unsigned long long* sw_small_scratch() {
    if constexpr (MEAS) {
        __shared__ unsigned long long s_scratch[7];
        return s_scratch;
    } else {
        return nullptr;
    }
}

struct SwMeasParams {  // one step's measuring passes on the multi-tile route (their own struct: SwParams stays as it is)
    const int8_t* s;
    const int* labels;
    unsigned long long* acc;  // per site: (up, down) counts of the sites gathered at this root, up in the low half; 0 elsewhere;
                              // then two words more, the step's frozen sites so far (n_frozen, m_frozen), 0 between steps
    unsigned long long* row;  // the step's 8 words, zeroed by the host
    long long sites;
    SwGeom g;
    int* err;
};

// One site's spin into its root's dword of LDS counts (up in the low 16 bits, down in the high 16: a workgroup's lattice or tile
// holds at most 16384 sites); a frozen site (root < 0, which has no slot) into frozen[0] (up) / frozen[1] (down).  Below T_c nearly
// every lane of a wave holds the same root, so the lanes of a wave that agree on it add as one: a single LDS atomic per wave instead
// of 64 on one address.  Every lane of the wave calls it together; `valid` masks the lanes without a site.
__device__ __forceinline__ void sw_tally(unsigned* cnt, unsigned* frozen, bool valid, int root, int spin) {
    const unsigned long long act = __ballot(valid);
    if (act == 0) return;
    const unsigned long long up = __ballot(valid && spin > 0), fz = __ballot(valid && root < 0), fr = act & ~fz;
    const int lane = (int)(threadIdx.x & 63u);
    if (fz != 0 && lane == __ffsll(fz) - 1) {
        if (fz & up) atomicAdd(&frozen[0], (unsigned)__popcll(fz & up));
        if (fz & ~up) atomicAdd(&frozen[1], (unsigned)__popcll(fz & ~up));
    }
    if (fr == 0) return;
    const int lead = __ffsll(fr) - 1;
    const int r0 = __shfl(root, lead);
    const unsigned long long same = __ballot(valid && root == r0);
    if (same == fr) {
        if (lane == lead) atomicAdd(&cnt[r0], (unsigned)__popcll(fr & up) | ((unsigned)__popcll(fr & ~up) << 16));
    } else if (valid && root >= 0) {
        atomicAdd(&cnt[root], spin > 0 ? 1u : 0x10000u);
    }
}

struct SwRowSum {  // words 0 .. 5 of a row, as one lane, wave or workgroup has them so far
    unsigned long long n, largest, s2, m2, m4lo, m4hi;
};

// a free cluster of `up` up spins and `dn` down spins (both below 2^31: |C|^2 and M_C^2 stay below 2^62, M_C^4 needs the high word)
__device__ __forceinline__ void sw_row_add(SwRowSum& a, unsigned up, unsigned dn) {
    const unsigned long long size = (unsigned long long)up + dn;
    const long long m = (long long)up - (long long)dn;
    const unsigned long long m2 = (unsigned long long)(m * m), lo = m2 * m2;
    a.n += 1;
    a.largest = size > a.largest ? size : a.largest;
    a.s2 += size * size;
    a.m2 += m2;
    a.m4lo += lo;
    a.m4hi += __umul64hi(m2, m2) + (a.m4lo < lo ? 1ull : 0ull);
}

// a 128-bit add into two 64-bit words by atomics: the returned old low word tells whether this add wrapped it
__device__ __forceinline__ void sw_add128(unsigned long long* lo_hi, unsigned long long lo, unsigned long long hi) {
    const unsigned long long old = atomicAdd(&lo_hi[0], lo);
    const unsigned long long carry = old + lo < lo ? 1ull : 0ull;
    if (hi + carry != 0) atomicAdd(&lo_hi[1], hi + carry);
}

// every lane's sums -> s_row[6] in LDS (zeroed, a barrier since): a wave reduction by shuffles, then one lane per wave.  All lanes of
// the workgroup call it; the caller's next barrier completes s_row
__device__ __forceinline__ void sw_row_block(SwRowSum a, unsigned long long* s_row) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        a.n += __shfl_xor(a.n, d);
        const unsigned long long l = __shfl_xor(a.largest, d);
        a.largest = l > a.largest ? l : a.largest;
        a.s2 += __shfl_xor(a.s2, d);
        a.m2 += __shfl_xor(a.m2, d);
        const unsigned long long lo = __shfl_xor(a.m4lo, d), hi = __shfl_xor(a.m4hi, d);
        a.m4lo += lo;
        a.m4hi += hi + (a.m4lo < lo ? 1ull : 0ull);
    }
    if ((threadIdx.x & 63u) == 0 && a.n != 0) {
        atomicAdd(&s_row[0], a.n);
        atomicMax(&s_row[1], a.largest);
        atomicAdd(&s_row[2], a.s2);
        atomicAdd(&s_row[3], a.m2);
        sw_add128(s_row + 4, a.m4lo, a.m4hi);
    }
}

// One-workgroup route, after the finds of a step (a barrier since): a root is a site with lab[i] == i, cnt holds its counts, fz the
// frozen sites'.  Writes the step's row and clears s_row and fz for the next step.  The row is this workgroup's alone: plain stores
__device__ __forceinline__ void sw_small_row(const int* lab, const unsigned* cnt, unsigned* fz, unsigned long long* s_row, int n,
                                             long long* row) {
    SwRowSum a = {};
    for (int i = threadIdx.x; i < n; i += blockDim.x)
        if (lab[i] == i) sw_row_add(a, cnt[i] & 0xFFFFu, cnt[i] >> 16);
    sw_row_block(a, s_row);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 0; k < 6; ++k) {
            row[k] = (long long)s_row[k];
            s_row[k] = 0;
        }
        row[6] = (long long)fz[0] + (long long)fz[1];
        row[7] = (long long)fz[0] - (long long)fz[1];
        fz[0] = fz[1] = 0;
    }
}

// Multi-tile route, pass 1, after the local pass (every label is its site's tile root, -1 where that root is frozen): one workgroup
// of 256 lanes per tile counts per tile root in LDS (one dword a site of the tile) and writes every site's acc word: the counts at
// a tile root, 0 elsewhere.  Frozen sites go to the two words behind acc, two atomics a workgroup.  One global atomic per site on
// its cluster's root instead would put most of an ordered lattice on a single word.
template <int DIM>
__global__ __launch_bounds__(256) void sw_meas_count(SwMeasParams p) {
    extern __shared__ unsigned s_cnt[];
    __shared__ unsigned s_fz[2];
    const SwGeom& g = p.g;
    const int TZ = DIM == 3 ? g.tz : 1, TR = g.tr, TC = g.tc, n = TZ * TR * TC;
    const int bz = DIM == 3 ? (int)(blockIdx.x / (unsigned)(g.nr * g.nc)) : 0, brc = (int)blockIdx.x - bz * g.nr * g.nc;
    const int br = brc / g.nc, bc = brc - br * g.nc;
    const int z0 = bz * TZ, r0 = br * TR, c0 = bc * TC;
    const int depth = DIM == 3 ? g.depth : 1;
    const int tz = depth - z0 < TZ ? depth - z0 : TZ, tr = g.rows - r0 < TR ? g.rows - r0 : TR, tc = g.cols - c0 < TC ? g.cols - c0 : TC;
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += 256) s_cnt[i] = 0;
    if (tid < 2) s_fz[tid] = 0;
    __syncthreads();
    bool bad = false;
    for (int base = 0; base < n; base += 256) {  // whole waves stay in the loop: sw_tally is a wave's call
        const int i = base + tid;
        const int lz = i / (TR * TC), rem = i - lz * TR * TC, lr = rem / TC, lc = rem - lr * TC;
        bool valid = i < n && lz < tz && lr < tr && lc < tc;
        int root = 0, spin = 0;
        if (valid) {
            const long long rho = (long long)(z0 + lz) * g.rows + r0 + lr;
            spin = p.s[rho * g.pitch + c0 + lc];
            const int lab = p.labels[rho * g.cols + c0 + lc];
            if (lab < 0) {
                root = -1;
            } else {  // the root's global index -> its index in the tile
                const int grho = lab / g.cols, gc = lab - grho * g.cols;
                const int gz = DIM == 3 ? grho / g.rows : 0, gr = grho - gz * g.rows;
                root = ((gz - z0) * TR + gr - r0) * TC + gc - c0;
                if (gz < z0 || gr < r0 || gc < c0 || gz - z0 >= tz || gr - r0 >= tr || gc - c0 >= tc) {  // not a label of the local pass
                    bad = true;
                    valid = false;
                }
            }
        }
        sw_tally(s_cnt, s_fz, valid, root, spin);
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int lz = i / (TR * TC), rem = i - lz * TR * TC, lr = rem / TC, lc = rem - lr * TC;
        if (lz >= tz || lr >= tr || lc >= tc) continue;
        const unsigned v = s_cnt[i];
        p.acc[((long long)(z0 + lz) * g.rows + r0 + lr) * g.cols + c0 + lc] = (unsigned long long)(v & 0xFFFFu) | ((unsigned long long)(v >> 16) << 32);
    }
    if (tid == 0 && (s_fz[0] | s_fz[1]) != 0) {
        atomicAdd(&p.acc[p.sites], (unsigned long long)s_fz[0] + s_fz[1]);
        atomicAdd(&p.acc[p.sites + 1], (unsigned long long)((long long)s_fz[0] - (long long)s_fz[1]));
    }
    if (bad) raise_err(p.err);
}

// Pass 2, after the merge pass: a tile root (acc != 0) that is no global root hands its counts to the root its chain ends in, one
// global atomic per tile root, or to the frozen words behind acc where the chain ends in the ghost.  Only global roots receive, and their own acc
// word is never 0, so no lane mistakes a word in flight.  256 lanes a workgroup, a grid-stride loop over the sites.  A percolating
// cluster has many tile roots a tile (the pieces that hang on it through a neighbouring tile only, a site per seam bond at worst),
// all bound for one word: the lanes of a wave that share the root of the wave's first sender add as one; the others send their own
template <int DIM>
__global__ __launch_bounds__(256) void sw_meas_fold(SwMeasParams p) {
    unsigned long long fu = 0, fd = 0;
    bool bad = false;
    const int lane = (int)(threadIdx.x & 63u);
    for (long long base = (long long)blockIdx.x * 256; base < p.sites; base += (long long)gridDim.x * 256) {  // whole waves stay in
        const long long i = base + threadIdx.x;
        unsigned long long a = i < p.sites ? p.acc[i] : 0;
        int r = -1;
        bool send = false;
        if (a != 0) {
            r = sw_chase<true>(p.labels, (int)i, bad);
            if (r < 0) {
                fu += a & 0xFFFFFFFFull;
                fd += a >> 32;
            } else {
                send = r != (int)i;
            }
        }
        const unsigned long long senders = __ballot(send);
        if (senders == 0) continue;
        const int lead = __ffsll(senders) - 1;
        const int r0 = __shfl(r, lead);
        const bool joins = send && r == r0;
        unsigned long long sum = joins ? a : 0;  // both halves stay below 2^31: no carry between them
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
        if (lane == lead) atomicAdd(&p.acc[r0], sum);
        if (send && !joins) atomicAdd(&p.acc[r], a);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        fu += __shfl_xor(fu, d);
        fd += __shfl_xor(fd, d);
    }
    if ((threadIdx.x & 63u) == 0 && (fu | fd) != 0) {
        atomicAdd(&p.acc[p.sites], fu + fd);
        atomicAdd(&p.acc[p.sites + 1], fu - fd);
    }
    if (bad) raise_err(p.err);
}

// Pass 3: the global roots (label == own index) form the row: a workgroup reduction, then at most six integer atomics a
// workgroup; workgroup 0 also moves the frozen words into the row.  A step whose cap expired (the error flag is up) leaves its row zero
template <int DIM>
__global__ __launch_bounds__(256) void sw_meas_row(SwMeasParams p) {
    __shared__ unsigned long long s_row[6];
    if (threadIdx.x < 6) s_row[threadIdx.x] = 0;
    __syncthreads();
    SwRowSum a = {};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < p.sites; i += (long long)gridDim.x * 256) {
        if (p.labels[i] != (int)i) continue;
        const unsigned long long v = p.acc[i];
        sw_row_add(a, (unsigned)(v & 0xFFFFFFFFull), (unsigned)(v >> 32));
    }
    sw_row_block(a, s_row);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const bool ok = __hip_atomic_load(p.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0;
    if (blockIdx.x == 0) {  // the frozen sites of passes 1 and 2 (both complete), and their words cleared for the next step
        if (ok) {
            p.row[6] = p.acc[p.sites];
            p.row[7] = p.acc[p.sites + 1];
        }
        p.acc[p.sites] = p.acc[p.sites + 1] = 0;
    }
    if (ok && s_row[0] != 0) {
        atomicAdd(&p.row[0], s_row[0]);
        atomicMax(&p.row[1], s_row[1]);
        atomicAdd(&p.row[2], s_row[2]);
        atomicAdd(&p.row[3], s_row[3]);
        sw_add128(p.row + 4, s_row[4], s_row[5]);
    }
}

}  // namespace

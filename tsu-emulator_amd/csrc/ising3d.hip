// ising3d.hip -- K8: heat-bath sweeps of a 3-D (cubic) lattice with per-bond couplings and per-site fields (gfx950).
//
// Site (z, r, c) of a D x R x C lattice of +-1 int8 spins, row-major with c fastest.  fp32 arrays of shape (D, R, C):
// J_right[z,r,c] couples (z,r,c)-(z,r,c+1), J_down[z,r,c] couples (z,r,c)-(z,r+1,c), J_layer[z,r,c] couples (z,r,c)-(z+1,r,c),
// h[z,r,c] is the site's field.  One periodic flag per axis (p_z, p_r, p_c); a periodic axis wraps to index 0 and has an even
// length >= 4, on an open axis the last slice of that axis's J is 0.  Device copies: rows of `pitch` elements (cols rounded up
// to 16: every row starts 16-byte aligned), pad columns 0, row rho = z R + r at rho * pitch.
// Decision rule (the bit-exact contract; physical mode):
//   colour of a site = (z + r + c) & 1; sweep t = half-sweep hs = 2 t (colour 0), then hs = 2 t + 1 (colour 1);
//   f   = ((((((J_layer[z-1] s[z-1]) + J_layer[z] s[z+1]) + J_down[r-1] s[r-1]) + J_down[r] s[r+1]) + J_right[c-1] s[c-1])
//         + J_right[c] s[c+1]) + h in float64, a neighbour missing on an open axis skipped (no +0.0);
//   x = 2 f / T;  p = sigmoid(x) clamped at +-20;  thr = floor(p 2^32 + 1/2);  the site becomes +1 iff u < thr;
//   u   = K1's 32-bit site uniform with the global row rho = z R + r in place of r: hi16 = half (m & 1) of
//         Philox(c >> 4, rho, hs, TAG_ISING_HI | replica << 8)[m >> 1] ^ 0x8000, m = (c >> 1) & 7, key = seed; lo16 from
//         TAG_ISING_LO, drawn only when hi16 ties with thr's top 16 bits.  No new tag.
// With D = 1 and p_z = 0 the z terms vanish, rho = r, and the rule is K7's: the spins equal tsu_ising2d_disorder_sweep's.
// randomize gives the spins tsu_ising2d_randomize gives a (D R) x C lattice.
//
// k8_sweep: one launch per half-sweep, in place (a colour reads only the other colour), one lane per octet (16 consecutive
// columns of one row rho = 8 sites of the colour = one Philox block).  A row takes L = min(64, the power of two >= ceil(C / 16))
// lanes, a workgroup of 256 lanes 256 / L consecutive rows; its even local rows go to waves 0 and 1, the odd ones to waves 2
// and 3, so the column parity (z + r + colour) & 1 is uniform in a wave except where a wave straddles two layers (the two
// parities are then taken one after the other; the result does not depend on it).  With C >= 1024 this is K7's shape: one row
// per wave.  The lane loads 16 bytes of its own row, of rows r -+ 1 of the layer and of the same row of layers z -+ 1, 16 floats
// of J_right, J_down, J_layer and h at the site and of J_down[r-1] and J_layer[z-1]; it screens its 8 sites in fp32 and takes
// the float64 threshold (and the lo16 block) only where the screen cannot decide (disorder_dev.h: the bound for seven terms, and the
// octet itself, Octet, shared with K7); one 16-byte store, the other colour's and the pad bytes written back as read.
//
// Bytes: a half-sweep reads every byte of the four arrays (16 B per site: a line holds both colours; J_down[r-1] and
// J_layer[z-1] are the own rows of other lanes of the launch and come from L2) and the spins (1 B per site from HBM, the four
// neighbour rows from L2), and writes 1 B per site: ~36 B per site and sweep.
//
// k8_energy + energy_final: E = -sum_bonds J s s' - sum h s in float64, a fixed number of per-workgroup partials then one
// workgroup summing them in a fixed order (the same bits on every call).  k8_sum / k8_overlap: sum s and q = sum s^a s^b
// (integers, one 64-bit vector atomic per workgroup).  The workgroup sums, the final sums and the pair lane are reduce_dev.h's,
// shared with K7.  No cooperative launch, no waiting, no atomics on the sweep path.
//
// Parallel tempering (tsu_pt3d_*): ladders of R walkers on ONE disorder ("Parallel tempering in 3-D (K8)").
// k8_pt_sweep is k8_sweep for a group of W walkers per lane (the walker group is the grid's z dimension): the octet's six
// couplings, field and screen bound are staged once (octet_group, disorder_dev.h) and every walker of the group takes k8_sweep's
// decision at the temperature of its slot, so the 32 B per site of disorder a sweep reads are shared by W walkers.  k8_pt_energy runs k8_energy's
// decomposition per walker through the same device helper (energy_lane: the bits of tsu_ising3d_energy) and sums the spins alongside.  The
// rest of a ladder does not know the dimension and is the 2-D ladders': the handle's tables and the host side of every entry point
// (pt_host.h), the final sums and q per slot (pt_energy_final, pt_overlap, reduce_dev.h) and the swap pass (pt_dev.h).  This file
// passes in how a half-sweep and an energy partial pass are launched.  No host value changes between rounds: a run of many rounds
// is enqueued without a synchronisation.
#include <cmath>
#include <cstdlib>
#include <new>
#include <vector>

#include "disorder_dev.h"
#include "ising2d.h"
#include "ising3d.h"
#include "corr_dev.h"
#include "pop_host.h"
#include "pt_host.h"
#include "pte_host.h"
#include "reduce_dev.h"

// Parallel tempering: pt_ladder.h's ladder with whole K8 lattices as its walkers, the 3-D counterpart of tsu_pt2d
struct tsu_pt3d : pt_ladder {
    tsu_ising3d** lat;  // walker g = ladder * R + w; lat[0] also holds the one disorder
};

// Population annealing: pop_host.h's population of K8 lattices, all planes in one allocation; `lat` owns the one disorder.  The
// sweeps and the energies are k8_pt_sweep and k8_pt_energy as they stand (every walker at slot 0, the schedule's tables offset by the
// step); the resampling kernels (pop_dev.h) are the 2-D populations' ("Population annealing")
struct tsu_pa3d : pop_handle {
    tsu_ising3d* lat;
};

// Tempering ensemble: pte_host.h's S samples x ladders of K8 lattices, all planes in one allocation and all disorder in another;
// `lat` gives the shape its checks and each sample's disorder its validation ("Tempering ensembles")
struct tsu_pte3d : pte_handle {
    tsu_ising3d* lat;
};

namespace {

struct K8Params {
    Geo g;            // J_right, J_down, J_layer, h
    Walker w;         // the spins, T, keys and tags
    uint32_t hs;
    long long nrows;  // depth * rows
    int lshift;       // log2 of the lanes per row
};

// The octet (Octet: loads, screen, exact branch, lo16 draw, store), the energy lane, Geo / Walker / PTParams / PTEns live in
// disorder_dev.h, the workgroup sums, the final sums, the pair lane and kEnergyBlocks in reduce_dev.h: all shared with K7

// (row rho, octet q) of a lane: grid (ceil(nrows / (256 >> lshift)), ceil(nchunks / 64)), 256 lanes.  Local row slot j of the
// workgroup's 256 >> lshift rows: the first half of the slots take the even local rows, the second half the odd ones.
template <class P>
__device__ __forceinline__ bool k8_lane(const P& p, long long& rho, int& q) {
    const int t = threadIdx.x;
    const int rpb = 256 >> p.lshift, half = rpb >> 1;
    const int j = t >> p.lshift;
    const int local = j < half ? 2 * j : 2 * (j - half) + 1;
    q = blockIdx.y * 64 + (t & ((1 << p.lshift) - 1));
    rho = (long long)blockIdx.x * rpb + local;
    return rho < p.nrows && 16 * q < p.g.cols;
}

// the same lane as (layer z, row r, octet q): what the sweeps take
template <class P>
__device__ __forceinline__ bool k8_lane(const P& p, int& z, int& r, int& q) {
    long long rho;
    if (!k8_lane(p, rho, q)) return false;
    z = (int)(rho / p.g.rows);
    r = (int)(rho - (long long)z * p.g.rows);
    return true;
}

__global__ __launch_bounds__(256) void k8_sweep(K8Params p, int colour) {
    int z, r, q;
    if (!k8_lane(p, z, r, q)) return;
    octet_single<3>(p.g, p.w, p.hs, z, r, q, colour);
}

// i.i.d. +-1: the bits of tsu_ising2d_randomize for a (depth * rows) x cols lattice (global row rho); pad bytes 0
__global__ __launch_bounds__(256) void k8_randomize(K8Params p, uint32_t tag) {
    long long rho;
    int q;
    if (!k8_lane(p, rho, q)) return;
    const u32x4 w = tsu_philox((uint32_t)(q >> 3), (uint32_t)rho, 0u, tag, p.w.k0, p.w.k1);
    const uint32_t wv[4] = {w.x, w.y, w.z, w.w};
    const uint32_t bits = (wv[(q & 7) >> 1] >> (16 * (q & 1))) & 0xFFFFu;
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = 4 * k + b;
            uint32_t byte = ((bits >> i) & 1u) ? 0x01u : 0xFFu;
            if (16 * q + i >= p.g.cols) byte = 0;
            v |= byte << (8 * b);
        }
        o[k] = v;
    }
    *reinterpret_cast<uint4*>(p.w.s + rho * p.g.pitch + 16 * q) = make_uint4(o[0], o[1], o[2], o[3]);
}

__global__ __launch_bounds__(256) void k8_fill(K8Params p, int value) {
    long long rho;
    int q;
    if (!k8_lane(p, rho, q)) return;
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t byte = (16 * q + 4 * k + b < p.g.cols) ? (uint32_t)(uint8_t)value : 0u;
            v |= byte << (8 * b);
        }
        o[k] = v;
    }
    *reinterpret_cast<uint4*>(p.w.s + rho * p.g.pitch + 16 * q) = make_uint4(o[0], o[1], o[2], o[3]);
}

// E partials: one per workgroup
__global__ __launch_bounds__(256) void k8_energy(K8Params p, double* __restrict__ part) {
    long long m;
    const double e = block_sum(energy_lane<3>(p.g, p.w.s, m));
    if (threadIdx.x == 0) part[blockIdx.x] = e;
}

// q = sum s^a s^b, one 64-bit vector atomic per workgroup
__global__ __launch_bounds__(256) void k8_overlap(const int8_t* __restrict__ a, const int8_t* __restrict__ b, long long pitch,
                                                  long long nrows, int cols, long long* __restrict__ acc) {
    const long long v = block_isum(pair_lane(a, b, pitch, pitch, nrows, cols));
    if (threadIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long*>(acc), (unsigned long long)v);
}

// sum s
__global__ __launch_bounds__(256) void k8_sum(const int8_t* __restrict__ a, long long pitch, long long nrows, int cols,
                                              long long* __restrict__ acc) {
    const long long v = block_isum(pair_lane(a, nullptr, pitch, pitch, nrows, cols));
    if (threadIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long*>(acc), (unsigned long long)v);
}

// ------------------------------------------------------------------ parallel tempering
// k8_sweep's grid with the walker group as its z dimension: lane = octet q of row rho (k8_lane) for the walkers of group z.
// The 64 staged floats and five spin vectors fit 255 VGPRs without scratch; the second launch bound keeps the allocator from
// spreading into AGPRs, which would halve the waves per SIMD for nothing.
__global__ __launch_bounds__(256, 2) void k8_pt_sweep(PTParams p, int colour) {
    int z, r, q;
    if (!k8_lane(p, z, r, q)) return;
    const int g0 = blockIdx.z * p.W;
    octet_group<3>(p, z, r, q, g0, min(g0 + p.W, p.nw), colour);
}

// k8_pt_sweep for an ensemble, a kernel of its own so that the ladders' code object stays what it was: the same lane and the same
// octet, for the walkers of one group of one sample on that sample's disorder.  The sample and its offsets are wave-uniform.
__global__ __launch_bounds__(256, 2) void k8_pte_sweep(PTParams p, PTEns e, int colour) {
    int z, r, q, g0, g1;
    if (!k8_lane(p, z, r, q)) return;
    pte_group(p, e, g0, g1);
    octet_group<3>(p, z, r, q, g0, g1, colour);
}

// grid (blocks_for(lattice), nw): workgroup x of walker y computes k8_energy's partial x of that walker alone, and its sum of spins
__global__ __launch_bounds__(256) void k8_pt_energy(PTParams p, double* __restrict__ part, long long* __restrict__ ipart) {
    long long m;
    const double e = energy_lane<3>(p.g, p.s[blockIdx.y], m);
    pt_energy_partials(e, m, part, ipart);
}

// k8_pt_energy for an ensemble: walker y on the disorder of its sample y / nper
__global__ __launch_bounds__(256) void k8_pte_energy(PTParams p, PTEns en, double* __restrict__ part, long long* __restrict__ ipart) {
    pte_sample(p.g, en, blockIdx.y / en.nper);
    long long m;
    const double e = energy_lane<3>(p.g, p.s[blockIdx.y], m);
    pt_energy_partials(e, m, part, ipart);
}

// the lattice's shape on the four disorder planes that start at `dis` (its own, or a sample's of an ensemble)
Geo make_geo(const tsu_ising3d* L, const float* dis) {
    const size_t plane = (size_t)L->depth * L->rows * L->pitch;
    Geo g = {};
    g.jr = dis;
    g.jd = dis ? dis + plane : nullptr;
    g.jl = dis ? dis + 2 * plane : nullptr;
    g.h = dis ? dis + 3 * plane : nullptr;
    g.pitch = (long long)L->pitch;
    g.depth = L->depth;
    g.rows = L->rows;
    g.cols = L->cols;
    g.pz = L->pz;
    g.pr = L->pr;
    g.pc = L->pc;
    return g;
}

// k8_lane's mapping for the lattice: nrows and the lanes per row, into a K8Params or a PTParams
template <class P>
void set_lanes(P& p, const tsu_ising3d* L) {
    const int nchunks = (L->cols + 15) >> 4;
    p.nrows = (long long)L->depth * L->rows;
    p.lshift = 0;
    while (p.lshift < 6 && (1 << p.lshift) < nchunks) ++p.lshift;
}

K8Params make_params(const tsu_ising3d* L) {
    K8Params p = {};
    p.g = make_geo(L, L->d_dis);
    p.w.s = L->s;
    set_lanes(p, L);
    return p;
}

// grid of the lane-per-octet kernels (k8_lane), with `groups` walker groups (or samples x groups) as its z dimension
template <class P>
dim3 octet_grid(const P& p, unsigned groups = 1) {
    const long long rpb = 256 >> p.lshift;
    const int nchunks = (p.g.cols + 15) >> 4;
    return dim3((unsigned)((p.nrows + rpb - 1) / rpb), (unsigned)((nchunks + 63) / 64), groups);
}

// the shape a ladder, an ensemble or a population keeps of its lattices
template <class H>
void set_shape(H* P, const tsu_ising3d* L) {
    P->nrows = (long long)L->depth * L->rows;
    P->pitch = (long long)L->pitch;
    P->cols = L->cols;
    P->n_axes = 3;
    P->lrows = L->rows;
    P->axis_len[0] = L->depth;
    P->axis_len[1] = L->rows;
    P->axis_len[2] = L->cols;
    P->axis_per[0] = L->pz;
    P->axis_per[1] = L->pr;
    P->axis_per[2] = L->pc;
}

unsigned blocks_for(const tsu_ising3d* L) { return reduce_blocks((long long)L->depth * L->rows * ((L->cols + 15) / 16)); }

int read_acc(tsu_ising3d* L, int64_t* out) {
    tsu_ctx* ctx = L->ctx;
    TSU_HIP_TRY(ctx, hipGetLastError());
    int64_t h = 0;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(&h, L->d_acc, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *out = h;
    return ising3d_check_err(L);
}

void pt_free(tsu_pt3d* P) { pt_delete(P, tsu_ising3d_destroy); }

// the parameters of nw walkers at W per lane, on lattice L's shape and the disorder at `dis`
template <class H>
PTParams ladder_on(const H* P, const tsu_ising3d* L, const float* dis, int nw, int W) {
    PTParams p = ladder_params(P, make_geo(L, dis), nw, W);
    set_lanes(p, L);
    return p;
}

PTParams pt_params(const tsu_pt3d* P) { return ladder_on(P, P->lat[0], P->lat[0]->d_dis, P->nw, 1); }

// k8_pt_energy for nw walkers into d_part / d_ipart (asynchronous): the partial pass pt_host.h's and pop_host.h's energies take
template <class H>
auto pt_partials(H* P, int nw, const PTParams& p) {
    return [P, nw, &p](unsigned blocks) { k8_pt_energy<<<dim3(blocks, (unsigned)nw, 1), 256, 0, P->ctx->stream>>>(p, P->d_part, P->d_ipart); };
}

void pte_free(tsu_pte3d* P) { pte_delete(P, tsu_ising3d_destroy); }

// the ladders' parameters for an ensemble: sample 0's disorder (the kernels add the sample's offset), the walkers of all samples
PTParams pte_params(const tsu_pte3d* P) { return ladder_on(P, P->lat, P->d_dis, P->nw, 1); }

// k8_pte_energy into d_part / d_ipart (asynchronous)
auto pte_partials(tsu_pte3d* P, const PTParams& p, const PTEns& e) {
    return [P, &p, &e](unsigned blocks) {
        k8_pte_energy<<<dim3(blocks, (unsigned)P->nw, 1), 256, 0, P->ctx->stream>>>(p, e, P->d_part, P->d_ipart);
    };
}

void pa_free(tsu_pa3d* P) { pop_delete(P, tsu_ising3d_destroy); }

// the ladders' parameters for a population: walker -> plane, key and slot 0; T / c32 are set per step
PTParams pa_params(const tsu_pa3d* P) { return ladder_on(P, P->lat, P->lat->d_dis, P->R, pop_group(P)); }

// half-sweep hs of every walker at step k's temperature: what pop_host.h's init and run take
auto pa_sweep(tsu_pa3d* P, PTParams& p) {
    const dim3 grid = octet_grid(p, (unsigned)((P->R + p.W - 1) / p.W));
    return [P, &p, grid](uint32_t hs, int colour, int k) {
        p.hs = hs;
        p.T = P->d_T + k;
        p.c32 = P->d_c32 + k;
        k8_pt_sweep<<<grid, 256, 0, P->ctx->stream>>>(p, colour);
    };
}

}  // namespace

extern "C" {

int tsu_ising3d_create(tsu_ctx* ctx, int depth, int rows, int cols, int periodic_mask, tsu_ising3d** out) {
    TSU_ENTER(ctx);
    if (!ctx || !out) return TSU_E_INVALID;
    *out = nullptr;
    TSU_REQUIRE(ctx, depth >= 1 && rows >= 1 && cols >= 1, "ising3d: depth/rows/cols must be positive");
    TSU_REQUIRE(ctx, (periodic_mask & ~7) == 0, "ising3d: periodic_mask must be a combination of TSU_PERIODIC_Z / _R / _C, got %d",
                periodic_mask);
    TSU_REQUIRE(ctx, (long long)depth * rows < (1ll << 31) && cols <= (1 << 30), "ising3d: lattice too large for 32-bit counters");
    const int len[3] = {depth, rows, cols};
    const char* axis[3] = {"depth", "rows", "cols"};
    for (int a = 0; a < 3; ++a)
        if (((periodic_mask >> a) & 1) && ((len[a] & 1) || len[a] < 4))
            return tsu_fail(ctx, TSU_E_UNSUPPORTED, "ising3d: a periodic axis needs an even length >= 4 (%s = %d)", axis[a], len[a]);
    tsu_ising3d* L = new (std::nothrow) tsu_ising3d();
    if (!L) return tsu_fail(ctx, TSU_E_NOMEM, "ising3d: host allocation failed");
    L->ctx = ctx;
    L->depth = depth;
    L->rows = rows;
    L->cols = cols;
    L->pz = (periodic_mask >> 0) & 1;
    L->pr = (periodic_mask >> 1) & 1;
    L->pc = (periodic_mask >> 2) & 1;
    L->pitch = ((size_t)cols + 15) / 16 * 16;
    const size_t bytes = (size_t)depth * rows * L->pitch;
    hipError_t e = hipMalloc((void**)&L->s, bytes);
    if (e == hipSuccess) e = hipMemsetAsync(L->s, 0, bytes, ctx->stream);
    if (e == hipSuccess) e = hipMalloc((void**)&L->d_part, (kEnergyBlocks + 1) * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&L->d_acc, sizeof(long long));
    if (e != hipSuccess) {
        const int rc = tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "ising3d_create: %s (%zu bytes)",
                                hipGetErrorString(e), bytes);
        if (L->s) (void)hipFree(L->s);
        if (L->d_part) (void)hipFree(L->d_part);
        if (L->d_acc) (void)hipFree(L->d_acc);
        delete L;
        return rc;
    }
    *out = L;
    return TSU_OK;
}

int tsu_ising3d_destroy(tsu_ising3d* L) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_OK;
    (void)hipStreamSynchronize(L->ctx->stream);
    if (L->s) (void)hipFree(L->s);
    if (L->d_dis) (void)hipFree(L->d_dis);
    if (L->d_part) (void)hipFree(L->d_part);
    if (L->d_acc) (void)hipFree(L->d_acc);
    if (L->d_prof) (void)hipFree(L->d_prof);
    if (L->h_err) (void)hipHostFree(L->h_err);
    tsu_sw_scratch_free(L->sw);
    delete L;
    return TSU_OK;
}

int tsu_ising3d_set_spins(tsu_ising3d* L, const int8_t* host) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, host, "ising3d_set_spins: NULL input");
    TSU_HIP_TRY(ctx, hipMemcpy2DAsync(L->s, L->pitch, host, (size_t)L->cols, (size_t)L->cols, (size_t)L->depth * L->rows,
                                      hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int tsu_ising3d_get_spins(tsu_ising3d* L, int8_t* host) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, host, "ising3d_get_spins: NULL output");
    TSU_HIP_TRY(ctx, hipMemcpy2DAsync(host, (size_t)L->cols, L->s, L->pitch, (size_t)L->cols, (size_t)L->depth * L->rows,
                                      hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ising3d_check_err(L);
}

int tsu_ising3d_randomize(tsu_ising3d* L, uint64_t seed, uint32_t replica) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE_REPLICA(ctx, replica, "ising3d_randomize");
    K8Params p = make_params(L);
    p.w.k0 = (uint32_t)seed;
    p.w.k1 = (uint32_t)(seed >> 32);
    k8_randomize<<<octet_grid(p), 256, 0, ctx->stream>>>(p, TSU_TAG_INIT | (replica << 8));
    TSU_HIP_TRY(ctx, hipGetLastError());
    return TSU_OK;
}

int tsu_ising3d_fill(tsu_ising3d* L, int8_t value) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, value == 1 || value == -1, "ising3d_fill: value must be +1 or -1");
    const K8Params p = make_params(L);
    k8_fill<<<octet_grid(p), 256, 0, ctx->stream>>>(p, (int)value);
    TSU_HIP_TRY(ctx, hipGetLastError());
    return TSU_OK;
}

int tsu_ising3d_set_disorder(tsu_ising3d* L, const float* J_right, const float* J_down, const float* J_layer, const float* h) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, J_right && J_down && J_layer, "ising3d_set_disorder: J_right, J_down and J_layer are required (h may be NULL)");
    const int depth = L->depth, rows = L->rows, cols = L->cols;
    for (int z = 0; z < depth; ++z)
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c) {
                const size_t i = ((size_t)z * rows + r) * cols + c;
                TSU_REQUIRE(ctx, std::isfinite(J_right[i]) && std::isfinite(J_down[i]) && std::isfinite(J_layer[i]) && (!h || std::isfinite(h[i])),
                            "ising3d_set_disorder: non-finite value at site (%d, %d, %d)", z, r, c);
                TSU_REQUIRE(ctx, L->pc || c + 1 < cols || J_right[i] == 0.0f,
                            "ising3d_set_disorder: open axis: J_right[%d, %d, %d] (last column) must be 0, got %g", z, r, c, (double)J_right[i]);
                TSU_REQUIRE(ctx, L->pr || r + 1 < rows || J_down[i] == 0.0f,
                            "ising3d_set_disorder: open axis: J_down[%d, %d, %d] (last row) must be 0, got %g", z, r, c, (double)J_down[i]);
                TSU_REQUIRE(ctx, L->pz || z + 1 < depth || J_layer[i] == 0.0f,
                            "ising3d_set_disorder: open axis: J_layer[%d, %d, %d] (last layer) must be 0, got %g", z, r, c, (double)J_layer[i]);
            }
    int have_field = 0;
    if (h)
        for (size_t i = 0, n = (size_t)depth * rows * cols; i < n && !have_field; ++i) have_field = h[i] != 0.0f;
    const size_t nrows = (size_t)depth * rows, plane = nrows * L->pitch;
    if (!L->d_dis) {
        TSU_HIP_TRY(ctx, hipMalloc((void**)&L->d_dis, 4 * plane * sizeof(float)));
        TSU_HIP_TRY(ctx, hipMemsetAsync(L->d_dis, 0, 4 * plane * sizeof(float), ctx->stream));  // pad columns stay 0
    }
    const size_t dpitch = L->pitch * sizeof(float), w = (size_t)cols * sizeof(float);
    const float* src[3] = {J_right, J_down, J_layer};
    for (int k = 0; k < 3; ++k)
        TSU_HIP_TRY(ctx, hipMemcpy2DAsync(L->d_dis + k * plane, dpitch, src[k], w, w, nrows, hipMemcpyHostToDevice, ctx->stream));
    if (h) TSU_HIP_TRY(ctx, hipMemcpy2DAsync(L->d_dis + 3 * plane, dpitch, h, w, w, nrows, hipMemcpyHostToDevice, ctx->stream));
    else TSU_HIP_TRY(ctx, hipMemsetAsync(L->d_dis + 3 * plane, 0, plane * sizeof(float), ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    L->have_disorder = 1;
    L->have_field = have_field;
    return TSU_OK;
}

int tsu_ising3d_sweep(tsu_ising3d* L, double T, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, L->have_disorder, "ising3d_sweep: call tsu_ising3d_set_disorder first");
    TSU_REQUIRE(ctx, T > 0.0 && std::isfinite(T), "Temperature must be positive");
    TSU_REQUIRE(ctx, n_sweeps >= 0, "ising3d_sweep: n_sweeps must be >= 0");
    TSU_REQUIRE(ctx, (uint64_t)sweep0 + (uint64_t)n_sweeps <= (1ull << 31), "ising3d_sweep: sweep counter overflow");
    TSU_REQUIRE_REPLICA(ctx, replica, "ising3d_sweep");
    if (n_sweeps == 0) return TSU_OK;
    K8Params p = make_params(L);
    ising2d_set_keys(p.w, seed, replica);
    p.w.T = T;
    p.w.c32 = (float)(2.0 / T);
    const dim3 grid = octet_grid(p);
    for (int s = 0; s < n_sweeps; ++s)
        for (int colour = 0; colour < 2; ++colour) {
            p.hs = 2u * (sweep0 + (uint32_t)s) + (uint32_t)colour;
            k8_sweep<<<grid, 256, 0, ctx->stream>>>(p, colour);
            L->launches += 1;
        }
    TSU_HIP_TRY(ctx, hipGetLastError());
    return TSU_OK;
}

int tsu_ising3d_energy(tsu_ising3d* L, double* E) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, E, "ising3d_energy: NULL output");
    TSU_REQUIRE(ctx, L->have_disorder, "ising3d_energy: call tsu_ising3d_set_disorder first");
    const unsigned blocks = blocks_for(L);
    const K8Params p = make_params(L);
    k8_energy<<<blocks, 256, 0, ctx->stream>>>(p, L->d_part);
    energy_final<<<1, 256, 0, ctx->stream>>>(L->d_part, (int)blocks, L->d_part + kEnergyBlocks);
    TSU_HIP_TRY(ctx, hipGetLastError());
    double e = 0.0;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(&e, L->d_part + kEnergyBlocks, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *E = e;
    return ising3d_check_err(L);
}

int tsu_ising3d_sum_spins(tsu_ising3d* L, int64_t* sum_s) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, sum_s, "ising3d_sum_spins: NULL output");
    TSU_HIP_TRY(ctx, hipMemsetAsync(L->d_acc, 0, sizeof(long long), ctx->stream));
    k8_sum<<<blocks_for(L), 256, 0, ctx->stream>>>(L->s, (long long)L->pitch, (long long)L->depth * L->rows, L->cols, L->d_acc);
    return read_acc(L, sum_s);
}

int tsu_ising3d_overlap(tsu_ising3d* A, tsu_ising3d* B, int64_t* q) {
    TSU_ENTER(A ? A->ctx : nullptr);
    if (!A || !B) return TSU_E_INVALID;
    tsu_ctx* ctx = A->ctx;
    TSU_REQUIRE(ctx, q, "ising3d_overlap: NULL output");
    TSU_REQUIRE(ctx, B->ctx == ctx, "ising3d_overlap: the two lattices belong to different contexts");
    TSU_REQUIRE(ctx, A->depth == B->depth && A->rows == B->rows && A->cols == B->cols,
                "ising3d_overlap: shapes differ (%d x %d x %d against %d x %d x %d)", A->depth, A->rows, A->cols, B->depth, B->rows, B->cols);
    TSU_HIP_TRY(ctx, hipMemsetAsync(A->d_acc, 0, sizeof(long long), ctx->stream));
    k8_overlap<<<blocks_for(A), 256, 0, ctx->stream>>>(A->s, B->s, (long long)A->pitch, (long long)A->depth * A->rows, A->cols, A->d_acc);
    return read_acc(A, q);
}

int tsu_ising3d_link_overlap(tsu_ising3d* A, tsu_ising3d* B, int64_t* Lout, int64_t* n_bonds) {
    TSU_ENTER(A ? A->ctx : nullptr);
    if (!A || !B) return TSU_E_INVALID;
    tsu_ctx* ctx = A->ctx;
    TSU_REQUIRE(ctx, Lout && n_bonds, "ising3d_link_overlap: NULL output");
    TSU_REQUIRE(ctx, B->ctx == ctx, "ising3d_link_overlap: the two lattices belong to different contexts");
    TSU_REQUIRE(ctx, A->depth == B->depth && A->rows == B->rows && A->cols == B->cols,
                "ising3d_link_overlap: shapes differ (%d x %d x %d against %d x %d x %d)", A->depth, A->rows, A->cols, B->depth, B->rows,
                B->cols);
    TSU_REQUIRE(ctx, A->pz == B->pz && A->pr == B->pr && A->pc == B->pc, "ising3d_link_overlap: the periodic axes of the two lattices differ");
    LinkArgs la;
    const unsigned blocks = link_plan(la, (long long)A->pitch, (long long)B->pitch, (long long)A->depth * A->rows, A->rows, A->cols, A->pz, A->pr, A->pc);
    TSU_HIP_TRY(ctx, hipMemsetAsync(A->d_acc, 0, sizeof(long long), ctx->stream));
    link_pass<<<blocks, 256, 0, ctx->stream>>>(A->s, B->s, la, A->d_acc);
    *n_bonds = link_bonds(A->depth, A->rows, A->cols, A->pz, A->pr, A->pc);
    return read_acc(A, Lout);
}

int tsu_ising3d_profiles(tsu_ising3d* A, tsu_ising3d* B, int64_t* p_z, int64_t* p_r, int64_t* p_c) {
    TSU_ENTER(A ? A->ctx : nullptr);
    if (!A) return TSU_E_INVALID;
    tsu_ctx* ctx = A->ctx;
    TSU_REQUIRE(ctx, p_z && p_r && p_c, "ising3d_profiles: NULL output");
    if (B) {
        TSU_REQUIRE(ctx, B->ctx == ctx, "ising3d_profiles: the two lattices belong to different contexts");
        TSU_REQUIRE(ctx, A->depth == B->depth && A->rows == B->rows && A->cols == B->cols,
                    "ising3d_profiles: shapes differ (%d x %d x %d against %d x %d x %d)", A->depth, A->rows, A->cols, B->depth, B->rows,
                    B->cols);
    }
    const size_t n = (size_t)A->depth + (size_t)A->rows + (size_t)A->cols;
    if (!A->d_prof) TSU_HIP_TRY(ctx, hipMalloc((void**)&A->d_prof, n * sizeof(long long)));
    TSU_HIP_TRY(ctx, hipMemsetAsync(A->d_prof, 0, n * sizeof(long long), ctx->stream));
    ProfArgs pa;
    const dim3 grid = profile_plan(pa, (long long)A->pitch, B ? (long long)B->pitch : 0, (long long)A->depth * A->rows, A->rows, A->cols, 1, 1);
    profile_pass<<<grid, 256, 0, ctx->stream>>>(A->s, B ? B->s : nullptr, pa, A->d_prof);
    TSU_HIP_TRY(ctx, hipGetLastError());
    int64_t* out[3] = {p_z, p_r, p_c};
    const int len[3] = {A->depth, A->rows, A->cols};
    const long long* src = A->d_prof;
    for (int a = 0; a < 3; ++a) {
        TSU_HIP_TRY(ctx, hipMemcpyAsync(out[a], src, (size_t)len[a] * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        src += len[a];
    }
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ising3d_check_err(A);
}

int tsu_ising3d_launch_count(tsu_ising3d* L, uint64_t* n) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L || !n) return TSU_E_INVALID;
    *n = L->launches;
    return TSU_OK;
}

// ------------------------------------------------------------------ parallel tempering
int tsu_pt3d_create(tsu_ctx* ctx, int depth, int rows, int cols, int periodic_mask, int n_temps, int n_ladders, tsu_pt3d** out) {
    TSU_ENTER(ctx);
    if (!ctx || !out) return TSU_E_INVALID;
    return pt_create(
        ctx, "pt3d", n_temps, n_ladders, out,
        [=](tsu_ising3d** L) { return tsu_ising3d_create(ctx, depth, rows, cols, periodic_mask, L); },
        [](tsu_pt3d* P, int8_t** planes) {
            set_shape(P, P->lat[0]);
            for (int g = 0; g < P->nw; ++g) planes[g] = P->lat[g]->s;
        },
        pt_free);
}

int tsu_pt3d_destroy(tsu_pt3d* P) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_OK;
    (void)hipStreamSynchronize(P->ctx->stream);
    pt_free(P);
    return TSU_OK;
}

int tsu_pt3d_set_disorder(tsu_pt3d* P, const float* J_right, const float* J_down, const float* J_layer, const float* h) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    return tsu_ising3d_set_disorder(P->lat[0], J_right, J_down, J_layer, h);  // stored once, with walker 0's lattice
}

int tsu_pt3d_set_temperatures(tsu_pt3d* P, const double* T) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_set_temperatures(P, T) : TSU_E_INVALID;
}

int tsu_pt3d_init(tsu_pt3d* P, uint64_t seed, int initial) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    return pt_init(
        P, seed, initial,
        [=](int g, uint64_t s) {  // temperature_scan_3d's model g
            return initial == 0 ? tsu_ising3d_randomize(P->lat[g], s, 0) : tsu_ising3d_fill(P->lat[g], (int8_t)initial);
        },
        [] { return (int)TSU_OK; });
}

int tsu_pt3d_run(tsu_pt3d* P, int n_rounds, int swap_interval, int do_swap, int record) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    tsu_ising3d* L = P->lat[0];
    const int rc = pt_run_check(P, L->have_disorder, n_rounds, swap_interval);
    if (rc != TSU_OK) return rc;
    PTParams p = pt_params(P);
    p.W = pt_group(P);
    const dim3 grid = octet_grid(p, (unsigned)((P->nw + p.W - 1) / p.W));
    return pt_run(
        P, n_rounds, swap_interval, do_swap, record,
        [&](uint32_t hs, int colour) {
            p.hs = hs;
            k8_pt_sweep<<<grid, 256, 0, ctx->stream>>>(p, colour);
        },
        pt_partials(P, P->nw, p), [] { return (int)TSU_OK; });
}

int tsu_pt3d_history(tsu_pt3d* P, double* E, int64_t* M, int64_t* q, int32_t* walker) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_history(P, E, M, q, walker) : TSU_E_INVALID;
}

int tsu_pt3d_stats(tsu_pt3d* P, int64_t* attempts, int64_t* accepts, int64_t* round_trips, int32_t* walker_at_slot, uint64_t* sweep_count,
                   uint64_t* round_count) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_stats(P, attempts, accepts, round_trips, walker_at_slot, sweep_count, round_count) : TSU_E_INVALID;
}

int tsu_pt3d_energies(tsu_pt3d* P, double* E, int64_t* sum_s) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const PTParams p = pt_params(P);
    return pt_energies(P, P->lat[0]->have_disorder, E, sum_s, pt_partials(P, P->nw, p));
}

int tsu_pt3d_get_spins(tsu_pt3d* P, int ladder, int slot, int8_t* host) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    TSU_REQUIRE(P->ctx, host, "pt3d_get_spins: NULL output");
    int g = 0;
    const int rc = pt_at(P, ladder, slot, "get_spins", &g);
    return rc != TSU_OK ? rc : tsu_ising3d_get_spins(P->lat[g], host);
}

int tsu_pt3d_set_spins(tsu_pt3d* P, int ladder, int slot, const int8_t* host) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    TSU_REQUIRE(P->ctx, host, "pt3d_set_spins: NULL input");
    int g = 0;
    const int rc = pt_at(P, ladder, slot, "set_spins", &g);
    return rc != TSU_OK ? rc : tsu_ising3d_set_spins(P->lat[g], host);
}

int tsu_pt3d_launch_count(tsu_pt3d* P, uint64_t* n) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return pt_launch_count(P, n);
}

int tsu_pt3d_set_correlation(tsu_pt3d* P, int enable, const double* cos_z, const double* sin_z, const double* cos_r, const double* sin_r,
                             const double* cos_c, const double* sin_c) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const double* cs[3] = {cos_z, cos_r, cos_c};
    const double* sn[3] = {sin_z, sin_r, sin_c};
    return pt_set_correlation(P, enable, cs, sn);
}

int tsu_pt3d_history_modes(tsu_pt3d* P, double* modes) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_history_modes(P, modes) : TSU_E_INVALID;
}

int tsu_pt3d_profiles(tsu_pt3d* P, int slot, int64_t* p_z, int64_t* p_r, int64_t* p_c) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    int64_t* out[3] = {p_z, p_r, p_c};
    return pt_profiles(P, slot, out);
}

int tsu_pt3d_set_link_overlap(tsu_pt3d* P, int enable) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_set_link_overlap(P, enable) : TSU_E_INVALID;
}

int tsu_pt3d_history_link(tsu_pt3d* P, int64_t* L) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_history_link(P, L) : TSU_E_INVALID;
}

// ------------------------------------------------------------------ tempering ensembles
int tsu_pte3d_create(tsu_ctx* ctx, int depth, int rows, int cols, int periodic_mask, int n_samples, int n_temps, int n_ladders,
                     tsu_pte3d** out) {
    TSU_ENTER(ctx);
    if (!ctx || !out) return TSU_E_INVALID;
    return pte_create(
        ctx, "pte3d", n_samples, n_temps, n_ladders, out,
        [=](tsu_pte3d* P) {
            const int rc = tsu_ising3d_create(ctx, depth, rows, cols, periodic_mask, &P->lat);
            if (rc != TSU_OK) return rc;
            set_shape(P, P->lat);
            P->n_dis = 4;
            return (int)TSU_OK;
        },
        pte_free);
}

int tsu_pte3d_destroy(tsu_pte3d* P) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_OK;
    (void)hipStreamSynchronize(P->ctx->stream);
    pte_free(P);
    return TSU_OK;
}

int tsu_pte3d_set_disorder(tsu_pte3d* P, const float* J_right, const float* J_down, const float* J_layer, const float* h) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const float* src[4] = {J_right, J_down, J_layer, h};
    return pte_set_disorder(
        P, src, (size_t)P->nrows * P->cols, [](tsu_pte3d* E) { return E->lat->d_dis; },
        [](tsu_ising3d* L, const float* const* a) { return tsu_ising3d_set_disorder(L, a[0], a[1], a[2], a[3]); });
}

int tsu_pte3d_set_temperatures(tsu_pte3d* P, const double* T) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_set_temperatures(P, T) : TSU_E_INVALID;
}

int tsu_pte3d_init(tsu_pte3d* P, const uint64_t* seeds, int initial) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pte_init(P, seeds, initial) : TSU_E_INVALID;
}

int tsu_pte3d_run(tsu_pte3d* P, int n_rounds, int swap_interval, int do_swap, int record) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    const int rc = pt_run_check(P, P->have_disorder, n_rounds, swap_interval);
    if (rc != TSU_OK) return rc;
    PTParams p = pte_params(P);
    p.W = pt_group(P);
    const PTEns e = pte_ens(P, p.W);
    const dim3 grid = octet_grid(p, (unsigned)P->S * (unsigned)e.groups);
    return pt_run(
        P, n_rounds, swap_interval, do_swap, record,
        [&](uint32_t hs, int colour) {
            p.hs = hs;
            k8_pte_sweep<<<grid, 256, 0, ctx->stream>>>(p, e, colour);
        },
        pte_partials(P, p, e), [] { return (int)TSU_OK; });
}

int tsu_pte3d_history(tsu_pte3d* P, double* E, int64_t* M, int64_t* q, int32_t* walker) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_history(P, E, M, q, walker) : TSU_E_INVALID;
}

int tsu_pte3d_stats(tsu_pte3d* P, int64_t* attempts, int64_t* accepts, int64_t* round_trips, int32_t* walker_at_slot,
                    uint64_t* sweep_count, uint64_t* round_count) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_stats(P, attempts, accepts, round_trips, walker_at_slot, sweep_count, round_count) : TSU_E_INVALID;
}

int tsu_pte3d_energies(tsu_pte3d* P, double* E, int64_t* sum_s) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const PTParams p = pte_params(P);
    const PTEns e = pte_ens(P, 1);
    return pt_energies(P, P->have_disorder, E, sum_s, pte_partials(P, p, e));
}

int tsu_pte3d_get_spins(tsu_pte3d* P, int sample, int ladder, int slot, int8_t* host) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pte_get_spins(P, sample, ladder, slot, host) : TSU_E_INVALID;
}

int tsu_pte3d_set_spins(tsu_pte3d* P, int sample, int ladder, int slot, const int8_t* host) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pte_set_spins(P, sample, ladder, slot, host) : TSU_E_INVALID;
}

int tsu_pte3d_launch_count(tsu_pte3d* P, uint64_t* n) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return pt_launch_count(P, n);
}

int tsu_pte3d_set_correlation(tsu_pte3d* P, int enable, const double* cos_z, const double* sin_z, const double* cos_r,
                              const double* sin_r, const double* cos_c, const double* sin_c) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const double* cs[3] = {cos_z, cos_r, cos_c};
    const double* sn[3] = {sin_z, sin_r, sin_c};
    return pt_set_correlation(P, enable, cs, sn);
}

int tsu_pte3d_history_modes(tsu_pte3d* P, double* modes) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_history_modes(P, modes) : TSU_E_INVALID;
}

int tsu_pte3d_set_link_overlap(tsu_pte3d* P, int enable) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_set_link_overlap(P, enable) : TSU_E_INVALID;
}

int tsu_pte3d_history_link(tsu_pte3d* P, int64_t* L) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_history_link(P, L) : TSU_E_INVALID;
}

int tsu_pte3d_profiles(tsu_pte3d* P, int sample, int slot, int64_t* p_z, int64_t* p_r, int64_t* p_c) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    int64_t* out[3] = {p_z, p_r, p_c};
    return pt_profiles(P, slot, out, sample);
}

// ------------------------------------------------------------------ population annealing
int tsu_pa3d_create(tsu_ctx* ctx, int depth, int rows, int cols, int periodic_mask, int population, tsu_pa3d** out) {
    TSU_ENTER(ctx);
    if (!ctx || !out) return TSU_E_INVALID;
    return pop_create(
        ctx, "pa3d", population, out,
        [=](tsu_pa3d* P) {
            const int rc = tsu_ising3d_create(ctx, depth, rows, cols, periodic_mask, &P->lat);
            if (rc != TSU_OK) return rc;
            set_shape(P, P->lat);
            return (int)TSU_OK;
        },
        pa_free);
}

int tsu_pa3d_destroy(tsu_pa3d* P) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_OK;
    (void)hipStreamSynchronize(P->ctx->stream);
    pa_free(P);
    return TSU_OK;
}

int tsu_pa3d_set_disorder(tsu_pa3d* P, const float* J_right, const float* J_down, const float* J_layer, const float* h) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    P->have_E = 0;
    return tsu_ising3d_set_disorder(P->lat, J_right, J_down, J_layer, h);
}

int tsu_pa3d_set_schedule(tsu_pa3d* P, const double* betas, int n) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pop_set_schedule(P, betas, n) : TSU_E_INVALID;
}

int tsu_pa3d_init(tsu_pa3d* P, uint64_t seed, int initial_sweeps) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    PTParams p = pa_params(P);
    return pop_init(P, P->lat->have_disorder, seed, initial_sweeps, pa_sweep(P, p), pt_partials(P, P->R, p));
}

int tsu_pa3d_run(tsu_pa3d* P, int n_steps, int sweeps_per_step, int resample, int record) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const int rc = pop_run_check(P, P->lat->have_disorder, n_steps, sweeps_per_step);
    if (rc != TSU_OK) return rc;
    PTParams p = pa_params(P);
    return pop_run(P, n_steps, sweeps_per_step, resample, record, pa_sweep(P, p), pt_partials(P, P->R, p));
}

int tsu_pa3d_history(tsu_pa3d* P, double* E, int64_t* M, uint32_t* W, int32_t* parent, uint64_t* S, uint64_t* U, double* E_min) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pop_history(P, E, M, W, parent, S, U, E_min) : TSU_E_INVALID;
}

int tsu_pa3d_energies(tsu_pa3d* P, double* E, int64_t* sum_s) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const PTParams p = pa_params(P);
    return pop_energies(P, P->lat->have_disorder, E, sum_s, pt_partials(P, P->R, p));
}

int tsu_pa3d_get_spins(tsu_pa3d* P, int i, int8_t* host) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pop_get_spins(P, i, host) : TSU_E_INVALID;
}

int tsu_pa3d_set_spins(tsu_pa3d* P, int i, const int8_t* host) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pop_set_spins(P, i, host) : TSU_E_INVALID;
}

int tsu_pa3d_launch_count(tsu_pa3d* P, uint64_t* n) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return pop_launch_count(P, n);
}

int tsu_pa3d_set_overlap(tsu_pa3d* P, int enable, const double* cos_z, const double* sin_z, const double* cos_r, const double* sin_r,
                         const double* cos_c, const double* sin_c) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const double* cs[3] = {cos_z, cos_r, cos_c};
    const double* sn[3] = {sin_z, sin_r, sin_c};
    return pop_set_overlap(P, enable, cs, sn);
}

int tsu_pa3d_history_overlap(tsu_pa3d* P, int64_t* q, int64_t* L, double* modes) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pop_history_overlap(P, q, L, modes) : TSU_E_INVALID;
}

}  // extern "C"

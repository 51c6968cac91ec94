// ising2d_disorder.hip -- K7: heat-bath sweeps of a 2-D lattice with per-bond couplings and per-site fields (gfx950).
//
// Quenched disorder on the lattice handle: J_right[r][c] (bond (r, c)-(r, c+1), wrapping to column 0 on a periodic lattice),
// J_down[r][c] (bond (r, c)-(r+1, c), wrapping to row 0) and h[r][c], fp32, row-major.  Device copies use the spin buffer's
// pitch (in elements), pad columns 0.  Decision rule (the bit-exact contract):
//   f   = (((J_down[r-1][c] s_up + J_down[r][c] s_down) + J_right[r][c-1] s_left) + J_right[r][c] s_right) + h[r][c] in float64,
//         a missing neighbour of an open lattice skipped (no +0.0);  x = 2 f / T;  p = sigmoid(x) clamped at +-20;
//   thr = floor(p 2^32 + 1/2);  the site becomes +1 iff u < thr, u = K1's own 32-bit site uniform (same counters, same tags:
//         hi16 = half (m & 1) of Philox(c >> 4, r, hs, TAG_ISING_HI | replica << 8)[m >> 1] ^ 0x8000, m = (c >> 1) & 7; lo16
//         from TAG_ISING_LO, drawn only when hi16 ties with thr's top 16 bits).
// With the 25-entry table replaced by this per-site threshold, a constant dyadic (J, h) gives K1's spins bit for bit.
//
// k7_sweep: one launch per half-sweep, one lane per octet (16 consecutive columns of one row = 8 sites of the colour, the
// unit of one Philox block), 64 x 4 lanes per workgroup = one row per wave, so the column parity of the colour is uniform
// in a wave.  The lane screens its 8 sites in fp32 and only takes the float64 threshold of the contract where the fp32
// probability lies within a margin of the hi16 uniform (disorder_dev.h: the bound with screen, and the octet itself, Octet, which is
// K8's with the z terms compiled out).  The spins are updated in place (a colour reads only the other colour), 16-byte masked stores,
// pad bytes untouched.  Every whole lattice K1 takes runs here (one-row and one-column lattices included); slabs are refused.
//
// Bytes: per half-sweep the launch reads every byte of the three disorder rows it touches (12 B per site: the lines hold both
// colours) and the spins (~3 B per site, up / down rows from L2), writes 1 B per site: ~28 B per site and sweep against the
// 2 B + 12 B / s of a tile-resident design.
//
// k7_energy + energy_final: E = -sum_bonds J s s' - sum h s in float64, per-workgroup partials then one workgroup summing them in
// a fixed order (the same bits on every call).  k7_overlap: q = sum s^a s^b (integer, vector atomics).  The workgroup sums, the
// final sums and the pair lane are reduce_dev.h's, shared with K8; the link overlap (tsu_ising2d_link_overlap, the ladders' and the
// populations' rows) is link_dev.h's, a 2-D lattice being its one-layer case.
//
// Parallel tempering (tsu_pt2d_*): ladders of R walkers on ONE disorder ("Parallel tempering (K7)").
// k7_pt_sweep is k7_sweep for a group of W walkers per lane: the octet's disorder is loaded and its 8 sites are staged once
// (octet_group, disorder_dev.h) and every walker of the group takes K7's decision at the temperature of its slot (a device table the
// swap kernel keeps), so the 24 B per site of disorder a sweep reads are shared by W walkers.  k7_pt_energy runs k7_energy's
// decomposition per walker through the same device helper (energy_lane: the same bits as the single-lattice call) and sums the
// spins alongside.  The rest of a ladder does not know the dimension and is shared with the 3-D
// ladders: the handle's tables and the host side of every entry point (pt_host.h: create, init, the run loop, history, ..), the
// final sums and q per slot (pt_energy_final, pt_overlap, reduce_dev.h) and the swap pass (k7_pt_swap, pt_dev.h).  This file
// passes in how a half-sweep and an energy partial pass are launched, and the hook that ends a round's sweeps with the replica
// cluster moves of ising2d_icm.hip (pt2d_icm_*).  The handle itself is declared in ising2d_pt.h.
//
// Population annealing (tsu_pa2d_*): R walkers on ONE disorder annealed along a schedule of inverse temperatures, resampled on the
// device between the steps ("Population annealing").  The sweeps and the energies are k7_pt_sweep and
// k7_pt_energy as they stand: every walker sits at slot 0 and the kernels get the schedule's tables offset by the step.  The
// resampling kernels (pop_dev.h) and the host side (pop_host.h) do not know the dimension and are shared with ising3d.hip.
#include <cmath>
#include <cstdlib>
#include <vector>

#include "dense.h"
#include "disorder_dev.h"
#include "ising2d.h"
#include "ising2d_pt.h"
#include "corr_dev.h"
#include "link_dev.h"
#include "pop_host.h"
#include "pt_host.h"
#include "pte_host.h"
#include "reduce_dev.h"

// Population annealing: pop_host.h's population of K7 lattices, all planes in one allocation; `lat` owns the one disorder
struct tsu_pa2d : pop_handle {
    tsu_ising2d* lat;
};

// Tempering ensemble: pte_host.h's S samples x ladders of K7 lattices, all planes in one allocation and all disorder in another;
// `lat` gives the shape its checks and each sample's disorder its validation ("Tempering ensembles")
struct tsu_pte2d : pte_handle {
    tsu_ising2d* lat;
};

namespace {

struct K7Params {
    Geo g;      // J_right, J_down, h: row pitch = the spin buffer's
    Walker w;   // owned row 0 of the current spin buffer, T, keys and tags
    uint32_t hs;
};

// The octet (Octet: loads, screen, exact branch, lo16 draw, store), the energy lane, Geo / Walker / PTParams / PTEns live in
// disorder_dev.h, the workgroup sums, the final sums, the pair lane and kEnergyBlocks in reduce_dev.h: all shared with K8

// lane = octet q of row r: grid (ceil(nchunks / 64), ceil(rows / 4)), 64 x 4 lanes
__device__ __forceinline__ bool k7_lane(const Geo& g, int& r, int& q) {
    q = blockIdx.x * 64 + threadIdx.x;
    r = blockIdx.y * 4 + threadIdx.y;
    return r < g.rows && 16 * q < g.cols;
}

__global__ __launch_bounds__(256) void k7_sweep(K7Params p, int colour) {
    int r, q;
    if (k7_lane(p.g, r, q)) octet_single<2>(p.g, p.w, p.hs, 0, r, q, colour);
}

// E partials: one per workgroup
__global__ __launch_bounds__(256) void k7_energy(K7Params p, double* __restrict__ part) {
    long long m;
    const double e = block_sum(energy_lane<2>(p.g, p.w.s, m));
    if (threadIdx.x == 0) part[blockIdx.x] = e;
}

// q, one 64-bit vector atomic per workgroup
__global__ __launch_bounds__(256) void k7_overlap(const int8_t* __restrict__ a, const int8_t* __restrict__ b, long long pitch_a,
                                                  long long pitch_b, int rows, int cols, long long* __restrict__ acc) {
    const long long v = block_isum(pair_lane(a, b, pitch_a, pitch_b, rows, cols));
    if (threadIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long*>(acc), (unsigned long long)v);
}

// ------------------------------------------------------------------ parallel tempering
// the swap pass lives in pt_dev.h, the final sums and q per slot in reduce_dev.h, the host side in pt_host.h: shared with ising3d.hip

// grid (ceil(nchunks / 64), ceil(rows / 4), ceil(nw / W)), 64 x 4 lanes: lane = octet q of row r for the walkers of group z
__global__ __launch_bounds__(256) void k7_pt_sweep(PTParams p, int colour) {
    int r, q;
    if (!k7_lane(p.g, r, q)) return;
    const int g0 = blockIdx.z * p.W;
    octet_group<2>(p, 0, r, q, g0, min(g0 + p.W, p.nw), colour);
}

// k7_pt_sweep for an ensemble, a kernel of its own so that the ladders' code object stays what it was: the same lane and the same
// octet, for the walkers of one group of one sample on that sample's disorder.  The sample and its offsets are wave-uniform.
__global__ __launch_bounds__(256) void k7_pte_sweep(PTParams p, PTEns e, int colour) {
    int r, q, g0, g1;
    if (!k7_lane(p.g, r, q)) return;
    pte_group(p, e, g0, g1);
    octet_group<2>(p, 0, r, q, g0, g1, colour);
}

// grid (blocks_for(lattice), nw): workgroup x of walker y computes k7_energy's partial x of that walker alone, and its sum of spins
__global__ __launch_bounds__(256) void k7_pt_energy(PTParams p, double* __restrict__ part, long long* __restrict__ ipart) {
    long long m;
    const double e = energy_lane<2>(p.g, p.s[blockIdx.y], m);
    pt_energy_partials(e, m, part, ipart);
}

// k7_pt_energy for an ensemble: walker y on the disorder of its sample y / nper
__global__ __launch_bounds__(256) void k7_pte_energy(PTParams p, PTEns en, double* __restrict__ part, long long* __restrict__ ipart) {
    pte_sample(p.g, en, blockIdx.y / en.nper);
    long long m;
    const double e = energy_lane<2>(p.g, p.s[blockIdx.y], m);
    pt_energy_partials(e, m, part, ipart);
}

bool whole_lattice(const tsu_ising2d* L) { return L->ghost == 0 && L->row0 == 0 && L->total_rows == L->rows; }

// the lattice's shape on the three disorder planes that start at `dis` (its own, or a sample's of an ensemble)
Geo make_geo(const tsu_ising2d* L, const float* dis) {
    const size_t plane = (size_t)L->rows * L->pitch;
    Geo g = {};
    g.jr = dis;
    g.jd = dis ? dis + plane : nullptr;
    g.h = dis ? dis + 2 * plane : nullptr;
    g.pitch = (long long)L->pitch;
    g.depth = 1;
    g.rows = L->rows;
    g.cols = L->cols;
    g.pr = g.pc = L->periodic;
    return g;
}

K7Params make_params(const tsu_ising2d* L) {
    K7Params p = {};
    p.g = make_geo(L, L->d_dis);
    p.w.s = L->alloc[L->cur];
    return p;
}

// the shape a ladder, an ensemble or a population keeps of its lattices
template <class H>
void set_shape(H* P, const tsu_ising2d* L) {
    P->nrows = L->rows;
    P->pitch = (long long)L->pitch;
    P->cols = L->cols;
    P->n_axes = 2;
    P->lrows = L->rows;
    P->axis_len[0] = L->rows;
    P->axis_len[1] = L->cols;
    P->axis_per[0] = P->axis_per[1] = L->periodic;
}

unsigned blocks_for(const tsu_ising2d* L) { return reduce_blocks((long long)L->rows * ((L->cols + 15) / 16)); }

// grid of the sweeps: k7_lane's, with `groups` walker groups (or samples x groups) as its z dimension
dim3 sweep_grid(const Geo& g, unsigned groups) {
    const int nchunks = (g.cols + 15) >> 4;
    return dim3((unsigned)((nchunks + 63) / 64), (unsigned)((g.rows + 3) / 4), groups);
}

void pt_free(tsu_pt2d* P) {
    pt2d_icm_free(P);
    pt_delete(P, tsu_ising2d_destroy);
}

PTParams pt_params(const tsu_pt2d* P) { return ladder_params(P, make_geo(P->lat[0], P->lat[0]->d_dis), P->nw, 1); }

// k7_pt_energy for nw walkers into d_part / d_ipart (asynchronous): the partial pass pt_host.h's and pop_host.h's energies take
template <class H>
auto pt_partials(H* P, int nw, const PTParams& p) {
    return [P, nw, &p](unsigned blocks) { k7_pt_energy<<<dim3(blocks, (unsigned)nw, 1), 256, 0, P->ctx->stream>>>(p, P->d_part, P->d_ipart); };
}

void pte_free(tsu_pte2d* P) { pte_delete(P, tsu_ising2d_destroy); }

// the ladders' parameters for an ensemble: sample 0's disorder (the kernels add the sample's offset), the walkers of all samples
PTParams pte_params(const tsu_pte2d* P) { return ladder_params(P, make_geo(P->lat, P->d_dis), P->nw, 1); }

// k7_pte_energy into d_part / d_ipart (asynchronous)
auto pte_partials(tsu_pte2d* P, const PTParams& p, const PTEns& e) {
    return [P, &p, &e](unsigned blocks) {
        k7_pte_energy<<<dim3(blocks, (unsigned)P->nw, 1), 256, 0, P->ctx->stream>>>(p, e, P->d_part, P->d_ipart);
    };
}

void pa_free(tsu_pa2d* P) { pop_delete(P, tsu_ising2d_destroy); }

// the ladders' parameters for a population: walker -> plane, key and slot 0; T / c32 are set per step
PTParams pa_params(const tsu_pa2d* P) { return ladder_params(P, make_geo(P->lat, P->lat->d_dis), P->R, pop_group(P)); }

// half-sweep hs of every walker at step k's temperature: what pop_host.h's init and run take
auto pa_sweep(tsu_pa2d* P, PTParams& p) {
    const dim3 grid = sweep_grid(p.g, (unsigned)((P->R + p.W - 1) / p.W));
    return [P, &p, grid](uint32_t hs, int colour, int k) {
        p.hs = hs;
        p.T = P->d_T + k;
        p.c32 = P->d_c32 + k;
        k7_pt_sweep<<<grid, dim3(64, 4, 1), 0, P->ctx->stream>>>(p, colour);
    };
}

}  // namespace

extern "C" {

int tsu_ising2d_set_disorder(tsu_ising2d* L, const float* J_right, const float* J_down, const float* h) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, J_right && J_down, "ising2d_set_disorder: J_right and J_down are required (h may be NULL)");
    if (!whole_lattice(L)) return tsu_fail(ctx, TSU_E_UNSUPPORTED, "ising2d_set_disorder: whole lattices only (not a slab)");
    const int rows = L->rows, cols = L->cols;
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            const size_t i = (size_t)r * cols + c;
            TSU_REQUIRE(ctx, std::isfinite(J_right[i]) && std::isfinite(J_down[i]) && (!h || std::isfinite(h[i])),
                        "ising2d_set_disorder: non-finite value at site (%d, %d)", r, c);
            TSU_REQUIRE(ctx, L->periodic || c + 1 < cols || J_right[i] == 0.0f,
                        "ising2d_set_disorder: open lattice: J_right[%d, %d] (last column) must be 0, got %g", r, c, (double)J_right[i]);
            TSU_REQUIRE(ctx, L->periodic || r + 1 < rows || J_down[i] == 0.0f,
                        "ising2d_set_disorder: open lattice: J_down[%d, %d] (last row) must be 0, got %g", r, c, (double)J_down[i]);
        }
    const size_t plane = (size_t)rows * L->pitch;
    if (!L->d_dis) {
        TSU_HIP_TRY(ctx, hipMalloc((void**)&L->d_dis, 3 * plane * sizeof(float)));
        TSU_HIP_TRY(ctx, hipMemsetAsync(L->d_dis, 0, 3 * plane * sizeof(float), ctx->stream));  // pad columns stay 0
    }
    const size_t dpitch = L->pitch * sizeof(float), w = (size_t)cols * sizeof(float);
    TSU_HIP_TRY(ctx, hipMemcpy2DAsync(L->d_dis, dpitch, J_right, w, w, (size_t)rows, hipMemcpyHostToDevice, ctx->stream));
    TSU_HIP_TRY(ctx, hipMemcpy2DAsync(L->d_dis + plane, dpitch, J_down, w, w, (size_t)rows, hipMemcpyHostToDevice, ctx->stream));
    if (h) TSU_HIP_TRY(ctx, hipMemcpy2DAsync(L->d_dis + 2 * plane, dpitch, h, w, w, (size_t)rows, hipMemcpyHostToDevice, ctx->stream));
    else TSU_HIP_TRY(ctx, hipMemsetAsync(L->d_dis + 2 * plane, 0, plane * sizeof(float), ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    L->have_disorder = 1;
    return TSU_OK;
}

int tsu_ising2d_clear_disorder(tsu_ising2d* L) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    L->have_disorder = 0;  // the buffers stay for the next set_disorder (freed with the handle)
    return TSU_OK;
}

int tsu_ising2d_disorder_sweep(tsu_ising2d* L, double T, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, L->have_disorder, "ising2d_disorder_sweep: call tsu_ising2d_set_disorder first");
    TSU_REQUIRE(ctx, T > 0.0 && std::isfinite(T), "Temperature must be positive");
    TSU_REQUIRE(ctx, n_sweeps >= 0, "ising2d_sweep: n_sweeps must be >= 0");
    TSU_REQUIRE(ctx, (uint64_t)sweep0 + (uint64_t)n_sweeps <= (1ull << 31), "ising2d_sweep: sweep counter overflow");
    TSU_REQUIRE_REPLICA(ctx, replica, "ising2d_disorder_sweep");
    if (n_sweeps == 0) return TSU_OK;
    if (L->timing) TSU_HIP_TRY(ctx, hipEventRecord(L->ev0, ctx->stream));
    K7Params p = make_params(L);
    ising2d_set_keys(p.w, seed, replica);
    p.w.T = T;
    p.w.c32 = (float)(2.0 / T);
    const dim3 grid = sweep_grid(p.g, 1);
    for (int s = 0; s < n_sweeps; ++s)
        for (int colour = 0; colour < 2; ++colour) {
            p.hs = 2u * (sweep0 + (uint32_t)s) + (uint32_t)colour;
            k7_sweep<<<grid, dim3(64, 4, 1), 0, ctx->stream>>>(p, colour);
            L->dis_launches += 1;
        }
    TSU_HIP_TRY(ctx, hipGetLastError());
    if (L->timing) {
        TSU_HIP_TRY(ctx, hipEventRecord(L->ev1, ctx->stream));
        L->timed = 1;
    }
    return TSU_OK;
}

int tsu_ising2d_disorder_energy(tsu_ising2d* L, double* E) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L) return TSU_E_INVALID;
    tsu_ctx* ctx = L->ctx;
    TSU_REQUIRE(ctx, E, "ising2d_disorder_energy: NULL output");
    TSU_REQUIRE(ctx, L->have_disorder, "ising2d_disorder_energy: call tsu_ising2d_set_disorder first");
    const unsigned blocks = blocks_for(L);
    TSU_HIP_TRY(ctx, ising2d_grow(L->d_dis_part, L->dis_part_cap, (kEnergyBlocks + 1) * sizeof(double)));
    const K7Params p = make_params(L);
    k7_energy<<<blocks, 256, 0, ctx->stream>>>(p, L->d_dis_part);
    energy_final<<<1, 256, 0, ctx->stream>>>(L->d_dis_part, (int)blocks, L->d_dis_part + kEnergyBlocks);
    TSU_HIP_TRY(ctx, hipGetLastError());
    double e = 0.0;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(&e, L->d_dis_part + kEnergyBlocks, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *E = e;
    return ising2d_check_err(L);
}

int tsu_ising2d_overlap(tsu_ising2d* A, tsu_ising2d* B, int64_t* q) {
    TSU_ENTER(A ? A->ctx : nullptr);
    if (!A || !B) return TSU_E_INVALID;
    tsu_ctx* ctx = A->ctx;
    TSU_REQUIRE(ctx, q, "ising2d_overlap: NULL output");
    TSU_REQUIRE(ctx, B->ctx == ctx, "ising2d_overlap: the two lattices belong to different contexts");
    TSU_REQUIRE(ctx, A->rows == B->rows && A->cols == B->cols && A->total_rows == B->total_rows,
                "ising2d_overlap: shapes differ (%d x %d against %d x %d)", A->rows, A->cols, B->rows, B->cols);
    TSU_REQUIRE(ctx, whole_lattice(A) && whole_lattice(B), "ising2d_overlap: whole lattices only (not slabs)");
    TSU_HIP_TRY(ctx, hipMemsetAsync(A->d_obs, 0, sizeof(int64_t), ctx->stream));
    k7_overlap<<<blocks_for(A), 256, 0, ctx->stream>>>(A->alloc[A->cur], B->alloc[B->cur], (long long)A->pitch, (long long)B->pitch,
                                                       A->rows, A->cols, (long long*)A->d_obs);
    TSU_HIP_TRY(ctx, hipGetLastError());
    int64_t h = 0;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(&h, A->d_obs, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *q = h;
    int rc = ising2d_check_err(A);
    return rc != TSU_OK ? rc : ising2d_check_err(B);
}

int tsu_ising2d_profiles(tsu_ising2d* A, tsu_ising2d* B, int64_t* p_row, int64_t* p_col) {
    TSU_ENTER(A ? A->ctx : nullptr);
    if (!A) return TSU_E_INVALID;
    tsu_ctx* ctx = A->ctx;
    TSU_REQUIRE(ctx, p_row && p_col, "ising2d_profiles: NULL output");
    if (!whole_lattice(A) || (B && !whole_lattice(B))) return tsu_fail(ctx, TSU_E_UNSUPPORTED, "ising2d_profiles: whole lattices only (not slabs)");
    if (B) {
        TSU_REQUIRE(ctx, B->ctx == ctx, "ising2d_profiles: the two lattices belong to different contexts");
        TSU_REQUIRE(ctx, A->rows == B->rows && A->cols == B->cols, "ising2d_profiles: shapes differ (%d x %d against %d x %d)", A->rows,
                    A->cols, B->rows, B->cols);
    }
    const size_t n = (size_t)A->rows + (size_t)A->cols;
    TSU_HIP_TRY(ctx, ising2d_grow(A->d_prof, A->prof_cap, n * sizeof(long long)));
    TSU_HIP_TRY(ctx, hipMemsetAsync(A->d_prof, 0, n * sizeof(long long), ctx->stream));
    ProfArgs pa;
    const dim3 grid = profile_plan(pa, (long long)A->pitch, B ? (long long)B->pitch : 0, A->rows, A->rows, A->cols, 0, 1);
    profile_pass<<<grid, 256, 0, ctx->stream>>>(A->alloc[A->cur], B ? B->alloc[B->cur] : nullptr, pa, A->d_prof);
    TSU_HIP_TRY(ctx, hipGetLastError());
    TSU_HIP_TRY(ctx, hipMemcpyAsync(p_row, A->d_prof, (size_t)A->rows * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipMemcpyAsync(p_col, A->d_prof + A->rows, (size_t)A->cols * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const int rc = ising2d_check_err(A);
    return rc != TSU_OK || !B ? rc : ising2d_check_err(B);
}

int tsu_ising2d_link_overlap(tsu_ising2d* A, tsu_ising2d* B, int64_t* Lout, int64_t* n_bonds) {
    TSU_ENTER(A ? A->ctx : nullptr);
    if (!A || !B) return TSU_E_INVALID;
    tsu_ctx* ctx = A->ctx;
    TSU_REQUIRE(ctx, Lout && n_bonds, "ising2d_link_overlap: NULL output");
    TSU_REQUIRE(ctx, B->ctx == ctx, "ising2d_link_overlap: the two lattices belong to different contexts");
    if (!whole_lattice(A) || !whole_lattice(B)) return tsu_fail(ctx, TSU_E_UNSUPPORTED, "ising2d_link_overlap: whole lattices only (not slabs)");
    TSU_REQUIRE(ctx, A->rows == B->rows && A->cols == B->cols, "ising2d_link_overlap: shapes differ (%d x %d against %d x %d)", A->rows,
                A->cols, B->rows, B->cols);
    TSU_REQUIRE(ctx, A->periodic == B->periodic, "ising2d_link_overlap: one lattice is periodic and the other is open");
    LinkArgs la;
    const unsigned blocks = link_plan(la, (long long)A->pitch, (long long)B->pitch, A->rows, A->rows, A->cols, 0, A->periodic, A->periodic);
    TSU_HIP_TRY(ctx, hipMemsetAsync(A->d_obs, 0, sizeof(int64_t), ctx->stream));
    link_pass<<<blocks, 256, 0, ctx->stream>>>(A->alloc[A->cur], B->alloc[B->cur], la, (long long*)A->d_obs);
    TSU_HIP_TRY(ctx, hipGetLastError());
    int64_t h = 0;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(&h, A->d_obs, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *Lout = h;
    *n_bonds = link_bonds(1, A->rows, A->cols, 0, A->periodic, A->periodic);
    const int rc = ising2d_check_err(A);
    return rc != TSU_OK ? rc : ising2d_check_err(B);
}

int tsu_ising2d_disorder_launch_count(tsu_ising2d* L, uint64_t* n) {
    TSU_ENTER(L ? L->ctx : nullptr);
    if (!L || !n) return TSU_E_INVALID;
    *n = L->dis_launches;
    return TSU_OK;
}

// ------------------------------------------------------------------ parallel tempering
int tsu_pt2d_create(tsu_ctx* ctx, int rows, int cols, int periodic, int n_temps, int n_ladders, tsu_pt2d** out) {
    TSU_ENTER(ctx);
    if (!ctx || !out) return TSU_E_INVALID;
    return pt_create(
        ctx, "pt2d", n_temps, n_ladders, out,
        [=](tsu_ising2d** L) { return tsu_ising2d_create(ctx, rows, cols, periodic, L); },  // every whole lattice K7 takes
        [](tsu_pt2d* P, int8_t** planes) {
            set_shape(P, P->lat[0]);
            for (int g = 0; g < P->nw; ++g) planes[g] = P->lat[g]->alloc[P->lat[g]->cur];
        },
        pt_free);
}

int tsu_pt2d_destroy(tsu_pt2d* P) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_OK;
    (void)hipStreamSynchronize(P->ctx->stream);
    pt_free(P);
    return TSU_OK;
}

int tsu_pt2d_set_disorder(tsu_pt2d* P, const float* J_right, const float* J_down, const float* h) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    return tsu_ising2d_set_disorder(P->lat[0], J_right, J_down, h);  // stored once, with walker 0's lattice
}

int tsu_pt2d_set_temperatures(tsu_pt2d* P, const double* T) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const int rc = pt_set_temperatures(P, T);
    return rc != TSU_OK ? rc : pt2d_icm_slots(P);  // which slots take part in the cluster moves (nothing to do while they are off)
}

int tsu_pt2d_init(tsu_pt2d* P, uint64_t seed, int initial) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    return pt_init(
        P, seed, initial,
        [=](int g, uint64_t s) {  // temperature_scan's model g
            return initial == 0 ? tsu_ising2d_randomize(P->lat[g], s, 0) : tsu_ising2d_fill(P->lat[g], (int8_t)initial);
        },
        [P] { return pt2d_icm_reset(P); });
}

int tsu_pt2d_run(tsu_pt2d* P, int n_rounds, int swap_interval, int do_swap, int record) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    tsu_ising2d* L = P->lat[0];
    const int rc = pt_run_check(P, L->have_disorder, n_rounds, swap_interval);
    if (rc != TSU_OK) return rc;
    TSU_REQUIRE(ctx, (uint64_t)P->icm_passes + (uint64_t)n_rounds <= 0xFFFFFFFFull, "pt2d_run: cluster-pass counter overflow");
    PTParams p = pt_params(P);
    p.W = pt_group(P);
    const dim3 grid = sweep_grid(p.g, (unsigned)((P->nw + p.W - 1) / p.W));
    return pt_run(
        P, n_rounds, swap_interval, do_swap, record,
        [&](uint32_t hs, int colour) {
            p.hs = hs;
            k7_pt_sweep<<<grid, dim3(64, 4, 1), 0, ctx->stream>>>(p, colour);
        },
        pt_partials(P, P->nw, p),
        [P] {  // replica cluster moves
            return P->icm_every >= 1 && P->rounds % (uint32_t)P->icm_every == 0 ? pt2d_icm_enqueue(P) : (int)TSU_OK;
        });
}

int tsu_pt2d_history(tsu_pt2d* P, double* E, int64_t* M, int64_t* q, int32_t* walker) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_history(P, E, M, q, walker) : TSU_E_INVALID;
}

int tsu_pt2d_stats(tsu_pt2d* P, int64_t* attempts, int64_t* accepts, int64_t* round_trips, int32_t* walker_at_slot, uint64_t* sweep_count,
                   uint64_t* round_count) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_stats(P, attempts, accepts, round_trips, walker_at_slot, sweep_count, round_count) : TSU_E_INVALID;
}

int tsu_pt2d_energies(tsu_pt2d* P, double* E, int64_t* sum_s) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const PTParams p = pt_params(P);
    return pt_energies(P, P->lat[0]->have_disorder, E, sum_s, pt_partials(P, P->nw, p));
}

int tsu_pt2d_get_spins(tsu_pt2d* P, int ladder, int slot, int8_t* host) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    TSU_REQUIRE(P->ctx, host, "pt2d_get_spins: NULL output");
    int g = 0;
    const int rc = pt_at(P, ladder, slot, "get_spins", &g);
    return rc != TSU_OK ? rc : tsu_ising2d_get_spins(P->lat[g], host, 0, P->lat[g]->rows);
}

int tsu_pt2d_set_spins(tsu_pt2d* P, int ladder, int slot, const int8_t* host) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    TSU_REQUIRE(P->ctx, host, "pt2d_set_spins: NULL input");
    int g = 0;
    const int rc = pt_at(P, ladder, slot, "set_spins", &g);
    return rc != TSU_OK ? rc : tsu_ising2d_set_spins(P->lat[g], host, 0, P->lat[g]->rows);
}

int tsu_pt2d_launch_count(tsu_pt2d* P, uint64_t* n) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return pt_launch_count(P, n);
}

int tsu_pt2d_set_correlation(tsu_pt2d* P, int enable, const double* cos_row, const double* sin_row, const double* cos_col,
                             const double* sin_col) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const double* cs[2] = {cos_row, cos_col};
    const double* sn[2] = {sin_row, sin_col};
    return pt_set_correlation(P, enable, cs, sn);
}

int tsu_pt2d_history_modes(tsu_pt2d* P, double* modes) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_history_modes(P, modes) : TSU_E_INVALID;
}

int tsu_pt2d_profiles(tsu_pt2d* P, int slot, int64_t* p_row, int64_t* p_col) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    int64_t* out[2] = {p_row, p_col};
    return pt_profiles(P, slot, out);
}

int tsu_pt2d_set_link_overlap(tsu_pt2d* P, int enable) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_set_link_overlap(P, enable) : TSU_E_INVALID;
}

int tsu_pt2d_history_link(tsu_pt2d* P, int64_t* L) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_history_link(P, L) : TSU_E_INVALID;
}

// ------------------------------------------------------------------ tempering ensembles
int tsu_pte2d_create(tsu_ctx* ctx, int rows, int cols, int periodic, int n_samples, int n_temps, int n_ladders, tsu_pte2d** out) {
    TSU_ENTER(ctx);
    if (!ctx || !out) return TSU_E_INVALID;
    return pte_create(
        ctx, "pte2d", n_samples, n_temps, n_ladders, out,
        [=](tsu_pte2d* P) {  // every whole lattice K7 takes
            const int rc = tsu_ising2d_create(ctx, rows, cols, periodic, &P->lat);
            if (rc != TSU_OK) return rc;
            set_shape(P, P->lat);
            P->n_dis = 3;
            return (int)TSU_OK;
        },
        pte_free);
}

int tsu_pte2d_destroy(tsu_pte2d* P) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_OK;
    (void)hipStreamSynchronize(P->ctx->stream);
    pte_free(P);
    return TSU_OK;
}

int tsu_pte2d_set_disorder(tsu_pte2d* P, const float* J_right, const float* J_down, const float* h) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const float* src[3] = {J_right, J_down, h};
    return pte_set_disorder(
        P, src, (size_t)P->nrows * P->cols, [](tsu_pte2d* E) { return E->lat->d_dis; },
        [](tsu_ising2d* L, const float* const* a) { return tsu_ising2d_set_disorder(L, a[0], a[1], a[2]); });
}

int tsu_pte2d_set_temperatures(tsu_pte2d* P, const double* T) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_set_temperatures(P, T) : TSU_E_INVALID;
}

int tsu_pte2d_init(tsu_pte2d* P, const uint64_t* seeds, int initial) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pte_init(P, seeds, initial) : TSU_E_INVALID;
}

int tsu_pte2d_run(tsu_pte2d* P, int n_rounds, int swap_interval, int do_swap, int record) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    tsu_ctx* ctx = P->ctx;
    const int rc = pt_run_check(P, P->have_disorder, n_rounds, swap_interval);
    if (rc != TSU_OK) return rc;
    PTParams p = pte_params(P);
    p.W = pt_group(P);
    const PTEns e = pte_ens(P, p.W);
    const dim3 grid = sweep_grid(p.g, (unsigned)P->S * (unsigned)e.groups);
    return pt_run(
        P, n_rounds, swap_interval, do_swap, record,
        [&](uint32_t hs, int colour) {
            p.hs = hs;
            k7_pte_sweep<<<grid, dim3(64, 4, 1), 0, ctx->stream>>>(p, e, colour);
        },
        pte_partials(P, p, e), [] { return (int)TSU_OK; });
}

int tsu_pte2d_history(tsu_pte2d* P, double* E, int64_t* M, int64_t* q, int32_t* walker) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_history(P, E, M, q, walker) : TSU_E_INVALID;
}

int tsu_pte2d_stats(tsu_pte2d* P, int64_t* attempts, int64_t* accepts, int64_t* round_trips, int32_t* walker_at_slot,
                    uint64_t* sweep_count, uint64_t* round_count) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_stats(P, attempts, accepts, round_trips, walker_at_slot, sweep_count, round_count) : TSU_E_INVALID;
}

int tsu_pte2d_energies(tsu_pte2d* P, double* E, int64_t* sum_s) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const PTParams p = pte_params(P);
    const PTEns e = pte_ens(P, 1);
    return pt_energies(P, P->have_disorder, E, sum_s, pte_partials(P, p, e));
}

int tsu_pte2d_get_spins(tsu_pte2d* P, int sample, int ladder, int slot, int8_t* host) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pte_get_spins(P, sample, ladder, slot, host) : TSU_E_INVALID;
}

int tsu_pte2d_set_spins(tsu_pte2d* P, int sample, int ladder, int slot, const int8_t* host) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pte_set_spins(P, sample, ladder, slot, host) : TSU_E_INVALID;
}

int tsu_pte2d_launch_count(tsu_pte2d* P, uint64_t* n) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return pt_launch_count(P, n);
}

int tsu_pte2d_set_correlation(tsu_pte2d* P, int enable, const double* cos_row, const double* sin_row, const double* cos_col,
                              const double* sin_col) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const double* cs[3] = {cos_row, cos_col, nullptr};
    const double* sn[3] = {sin_row, sin_col, nullptr};
    return pt_set_correlation(P, enable, cs, sn);
}

int tsu_pte2d_history_modes(tsu_pte2d* P, double* modes) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_history_modes(P, modes) : TSU_E_INVALID;
}

int tsu_pte2d_set_link_overlap(tsu_pte2d* P, int enable) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_set_link_overlap(P, enable) : TSU_E_INVALID;
}

int tsu_pte2d_history_link(tsu_pte2d* P, int64_t* L) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pt_history_link(P, L) : TSU_E_INVALID;
}

int tsu_pte2d_profiles(tsu_pte2d* P, int sample, int slot, int64_t* p_row, int64_t* p_col) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    int64_t* out[3] = {p_row, p_col, nullptr};
    return pt_profiles(P, slot, out, sample);
}

// ------------------------------------------------------------------ population annealing
int tsu_pa2d_create(tsu_ctx* ctx, int rows, int cols, int periodic, int population, tsu_pa2d** out) {
    TSU_ENTER(ctx);
    if (!ctx || !out) return TSU_E_INVALID;
    return pop_create(
        ctx, "pa2d", population, out,
        [=](tsu_pa2d* P) {  // every whole lattice K7 takes
            const int rc = tsu_ising2d_create(ctx, rows, cols, periodic, &P->lat);
            if (rc != TSU_OK) return rc;
            set_shape(P, P->lat);
            return (int)TSU_OK;
        },
        pa_free);
}

int tsu_pa2d_destroy(tsu_pa2d* P) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_OK;
    (void)hipStreamSynchronize(P->ctx->stream);
    pa_free(P);
    return TSU_OK;
}

int tsu_pa2d_set_disorder(tsu_pa2d* P, const float* J_right, const float* J_down, const float* h) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    P->have_E = 0;
    return tsu_ising2d_set_disorder(P->lat, J_right, J_down, h);
}

int tsu_pa2d_set_schedule(tsu_pa2d* P, const double* betas, int n) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pop_set_schedule(P, betas, n) : TSU_E_INVALID;
}

int tsu_pa2d_init(tsu_pa2d* P, uint64_t seed, int initial_sweeps) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    PTParams p = pa_params(P);
    return pop_init(P, P->lat->have_disorder, seed, initial_sweeps, pa_sweep(P, p), pt_partials(P, P->R, p));
}

int tsu_pa2d_run(tsu_pa2d* P, int n_steps, int sweeps_per_step, int resample, int record) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const int rc = pop_run_check(P, P->lat->have_disorder, n_steps, sweeps_per_step);
    if (rc != TSU_OK) return rc;
    PTParams p = pa_params(P);
    return pop_run(P, n_steps, sweeps_per_step, resample, record, pa_sweep(P, p), pt_partials(P, P->R, p));
}

int tsu_pa2d_history(tsu_pa2d* P, double* E, int64_t* M, uint32_t* W, int32_t* parent, uint64_t* S, uint64_t* U, double* E_min) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pop_history(P, E, M, W, parent, S, U, E_min) : TSU_E_INVALID;
}

int tsu_pa2d_energies(tsu_pa2d* P, double* E, int64_t* sum_s) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const PTParams p = pa_params(P);
    return pop_energies(P, P->lat->have_disorder, E, sum_s, pt_partials(P, P->R, p));
}

int tsu_pa2d_get_spins(tsu_pa2d* P, int i, int8_t* host) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pop_get_spins(P, i, host) : TSU_E_INVALID;
}

int tsu_pa2d_set_spins(tsu_pa2d* P, int i, const int8_t* host) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pop_set_spins(P, i, host) : TSU_E_INVALID;
}

int tsu_pa2d_launch_count(tsu_pa2d* P, uint64_t* n) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return pop_launch_count(P, n);
}

int tsu_pa2d_set_overlap(tsu_pa2d* P, int enable, const double* cos_row, const double* sin_row, const double* cos_col, const double* sin_col) {
    TSU_ENTER(P ? P->ctx : nullptr);
    if (!P) return TSU_E_INVALID;
    const double* cs[2] = {cos_row, cos_col};
    const double* sn[2] = {sin_row, sin_col};
    return pop_set_overlap(P, enable, cs, sn);
}

int tsu_pa2d_history_overlap(tsu_pa2d* P, int64_t* q, int64_t* L, double* modes) {
    TSU_ENTER(P ? P->ctx : nullptr);
    return P ? pop_history_overlap(P, q, L, modes) : TSU_E_INVALID;
}

}  // extern "C"

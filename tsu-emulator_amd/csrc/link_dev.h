// link_dev.h -- the link overlap of two spin planes on one disorder ("Overlaps of walker pairs"):
// L = sum over bonds (i, j) of p_i p_j with p = s^a s^b, for lattice pairs, for every slot of a two-ladder tempering handle and
// for the walker pairs of a population.  Dimension-blind like reduce_dev.h and corr_dev.h: a plane is `nrows` rows of `pitch` bytes
// of which the first `cols` count, row rho = z lrows + r, one periodic flag per axis (a 2-D lattice: one layer, open z).  The bonds
// are the bonds of the energy passes (energy_lane, disorder_dev.h): every site's right, down and layer bond, the last bond of an
// open axis dropped, the wrap bond of a periodic axis kept, so an axis of length 1 or 2 counts its wrap as the energy does.
//
// Integers only.  Spins are the bytes 0x01 / 0xFF, so x = a ^ b is 0x00 (p = +1) or 0xFE (p = -1) per site and 0x00 on the pad
// bytes, and a bond is broken (p_i p_j = -1) exactly where bit 1 of x_i ^ x_j is set: a lane takes whole 16-byte chunks, xors
// them with the neighbour's chunk (the right neighbour: the chunk shifted down by one byte, its last byte from the next chunk's
// first dword), masks the bits of the bonds that exist and counts them with v_bcnt.  L = (bonds) - 2 (broken bonds).
//
// A lane keeps its chunk column over a band of `band` consecutive rows of one layer, so the down neighbour of a row is the chunk
// the next step needs anyway: the planes are loaded once per site plus once per band for the row below it.  The layer neighbour
// is a second read of both planes (one layer ahead, which another workgroup reads at about the same time); the wrap column of a
// periodic row costs the row's last chunk two byte loads.  Everything here has internal linkage.
#pragma once
#include "reduce_dev.h"

namespace {

struct LinkArgs {
    long long pitch_a, pitch_b, nrows;
    int lrows;       // rows of a layer (2-D: nrows)
    int cols;
    int band;        // consecutive rows a lane walks
    int pz, pr, pc;  // periodic flag of the layer, row and column axis
};

__device__ __forceinline__ uint4 link_x(const int8_t* __restrict__ a, const int8_t* __restrict__ b, const LinkArgs& p, long long rho,
                                        int c0) {
    const uint4 va = *reinterpret_cast<const uint4*>(a + rho * p.pitch_a + c0);
    const uint4 vb = *reinterpret_cast<const uint4*>(b + rho * p.pitch_b + c0);
    return make_uint4(va.x ^ vb.x, va.y ^ vb.y, va.z ^ vb.z, va.w ^ vb.w);
}

// set bits of (x ^ y) under the mask m: one per broken bond
__device__ __forceinline__ int link_broken(const uint4& x, const uint4& y, const uint32_t (&m)[4]) {
    return __popc((x.x ^ y.x) & m[0]) + __popc((x.y ^ y.y) & m[1]) + __popc((x.z ^ y.z) & m[2]) + __popc((x.w ^ y.w) & m[3]);
}

// a lane's share of L; lane = (layer z, band of rows, chunk q) with q fastest, grid-stride over blockIdx.x
__device__ __forceinline__ long long link_lane(const int8_t* __restrict__ a, const int8_t* __restrict__ b, const LinkArgs& p) {
    const int nchunks = (p.cols + 15) >> 4;
    const int bands = (p.lrows + p.band - 1) / p.band;
    const long long depth = p.nrows / p.lrows;
    const long long total = depth * bands * nchunks;
    long long sum = 0;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long zb = t / nchunks;
        const int q = (int)(t - zb * nchunks), c0 = 16 * q;
        const long long z = zb / bands;
        const int r0 = (int)(zb - z * bands) * p.band;
        const int rend = r0 + p.band < p.lrows ? r0 + p.band : p.lrows;
        // bit 1 of every byte whose column counts (m) and whose right neighbour is the next column of the row (mr)
        uint32_t m[4], mr[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int n = p.cols - (c0 + 4 * w);
            m[w] = n >= 4 ? 0x02020202u : (n <= 0 ? 0u : 0x02020202u & ((1u << (8 * n)) - 1u));
            mr[w] = n >= 5 ? 0x02020202u : (n <= 1 ? 0u : 0x02020202u & ((1u << (8 * (n - 1))) - 1u));
        }
        const int nsite = __popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]);
        const int nright = __popc(mr[0]) + __popc(mr[1]) + __popc(mr[2]) + __popc(mr[3]);
        const bool last = q == nchunks - 1;
        const bool wrap = p.pc && last;  // the chunk holds the last column, whose right neighbour is column 0
        const int iw = (p.cols - 1) & 15;
        const bool has_fw = z + 1 < depth || p.pz;
        long long rho = z * p.lrows + r0;
        uint4 x = link_x(a, b, p, rho, c0);
        int bonds = 0, broken = 0;
        for (int r = r0; r < rend; ++r, ++rho) {
            uint32_t nxt = 0;
            if (!last)
                nxt = *reinterpret_cast<const uint32_t*>(a + rho * p.pitch_a + c0 + 16) ^
                      *reinterpret_cast<const uint32_t*>(b + rho * p.pitch_b + c0 + 16);
            const uint4 y = make_uint4((x.x >> 8) | (x.y << 24), (x.y >> 8) | (x.z << 24), (x.z >> 8) | (x.w << 24), (x.w >> 8) | (nxt << 24));
            broken += link_broken(x, y, mr);
            bonds += nright;
            if (wrap) {
                const uint32_t word = iw < 8 ? (iw < 4 ? x.x : x.y) : (iw < 12 ? x.z : x.w);
                const uint32_t first = (uint32_t)(uint8_t)(a[rho * p.pitch_a] ^ b[rho * p.pitch_b]);
                broken += (int)((((word >> (8 * (iw & 3))) ^ first) >> 1) & 1u);
                bonds += 1;
            }
            const bool inside = r + 1 < p.lrows;
            uint4 xd = x;
            if (inside || p.pr) {
                xd = link_x(a, b, p, inside ? rho + 1 : z * p.lrows, c0);
                broken += link_broken(x, xd, m);
                bonds += nsite;
            }
            if (has_fw) {
                const uint4 xf = link_x(a, b, p, z + 1 < depth ? rho + p.lrows : (long long)r, c0);
                broken += link_broken(x, xf, m);
                bonds += nsite;
            }
            x = xd;  // the next row of the band (the band ends where the layer does)
        }
        sum += bonds - 2 * broken;
    }
    return sum;
}

// L of one plane pair, added into out[0] (zeroed): one 64-bit vector atomic per workgroup
__global__ __launch_bounds__(256) void link_pass(const int8_t* __restrict__ a, const int8_t* __restrict__ b, LinkArgs p,
                                                 long long* __restrict__ out) {
    const long long v = block_isum(link_lane(a, b, p));
    if (threadIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long*>(out), (unsigned long long)v);
}

// grid (blocks, S R): L of the two ladders' walkers of sample y / R at slot y % R (a population: one sample, the walkers y and
// y + R), added into out[y] (a zeroed history row [sample][slot]); the planes are found as pt_overlap finds them
__global__ __launch_bounds__(256) void pt_link(int8_t* const* __restrict__ s, const int32_t* __restrict__ was, int R, LinkArgs p,
                                               long long* __restrict__ out) {
    const int y = blockIdx.y, smp = y / R, i = y - smp * R;
    s += (size_t)smp * 2 * R;
    was += (size_t)smp * 2 * R;
    const long long v = block_isum(link_lane(s[was[i]], s[R + was[R + i]], p));
    if (threadIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long*>(out + y), (unsigned long long)v);
}

// The launch shape of a link pass: the workgroups per plane pair.  Bands of 8 rows where that still leaves a lane for every thread
// of 256 workgroups, else of 4, 2 or 1 rows: a small plane is served by the caches whatever the band, a large one reads its rows
// once plus one row in `band`.
inline unsigned link_plan(LinkArgs& p, long long pitch_a, long long pitch_b, long long nrows, int lrows, int cols, int pz, int pr,
                          int pc) {
    const long long nchunks = (cols + 15) / 16, depth = nrows / lrows;
    int band = 8;
    while (band > 1 && depth * ((lrows + band - 1) / band) * nchunks < 65536) band >>= 1;
    p.pitch_a = pitch_a;
    p.pitch_b = pitch_b;
    p.nrows = nrows;
    p.lrows = lrows;
    p.cols = cols;
    p.band = band;
    p.pz = pz;
    p.pr = pr;
    p.pc = pc;
    return reduce_blocks(depth * ((lrows + band - 1) / band) * nchunks);
}

// N_b: the bonds of a depth x lrows x cols lattice as the energy passes count them
inline long long link_bonds(long long depth, long long lrows, long long cols, int pz, int pr, int pc) {
    const long long n = depth * lrows * cols;
    return (pz ? n : n - n / depth) + (pr ? n : n - n / lrows) + (pc ? n : n - n / cols);
}

}  // namespace

// ising2d_tiled.hip -- K1 fast path: LDS-staged 2-D halo tiles, k full sweeps per launch (gfx950).
//
// Same Markov kernel and the same Philox stream as k1_generic / oracle ora_ising2d_sweep (results are bit
// identical); what changes is the schedule:
//   * a workgroup stages a (H + 4k) x (16 WO + 32) tile of the int8 lattice into LDS, de-interleaved into two
//     colour planes of 0/1 "up" flags (8 same-colour sites of a row = one octet = one uint64; 0/8 in the QUAD kernels),
//   * keeps the two planes interleaved row by row: behind the pair table of the compare and one guard octet, tile row r is its
//     NO = WO + 2 octets of plane 0 followed by its NO octets of plane 1, then one spare row and the 25 thresholds of the tie
//     path.  Row stride (2 NO octets) and plane distance (NO octets) are compile-time constants for a tile of any height, so the
//     pair loop carries ONE LDS address and every read and write of a pair is that address plus an immediate (see pair_step),
//   * runs 2k half-sweeps entirely in LDS (the region that is still exact shrinks by one site per half-sweep:
//     2k halo rows, one halo octet = 16 columns >= 2k each side), and
//   * writes the H x 16 WO interior to the OTHER lattice buffer (neighbouring tiles read this tile's pre-launch
//     halo, so the launch is out of place; the host ping-pongs).
// When every tile of the lattice has its own workgroup on the chip (up to 2^25 sites), k1_resident keeps the tiles in
// LDS for a whole call and only exchanges boundary strips between generations of k sweeps (see ResidentParams).
// HBM traffic is 2/k bytes per spin update instead of 2 (far less when resident); the kernel is VALU bound (Philox), so per octet:
//   one Philox4x32-10 block -> 8 x 16 random bits; neighbour sums with packed byte adds; the 16-bit thresholds of two
//   sites at a time from a 25-dword LDS table indexed by their two counts (v_dot4_u32_u8 + ds_read_b32; periodic byte planes
//   with 5 KB of LDS to spare: of four sites at a time from a 625-entry table, up-flags stored as 8, see pair_thresholds; open
//   lattices, whose edge sites have other degrees, pick them per site with v_perm_b32 byte look-ups); v_pk_sub_i16 (saturating) compares two
//   sites per instruction; only an exact tie of the top 16 bits (2^-16 per site) evaluates the low half.
// The form of the pair loop (plain / EDGE / SEAM / OPEN) and par0, the column parity of the colour updated in a half-sweep's first
// row, are fixed per tile: half-sweep hsi starts at tile row 1 + hsi and updates colour hsi & 1, whose sum is always odd, so par0
// depends on the parity of the window's first global row alone (odd only for a row slab that starts on an odd row).  Both are
// decided once per tile; the half-sweeps run two per trip, colour 0 then colour 1, with the colour a template parameter.
#include "ising2d.h"

#include <type_traits>
#include <vector>

typedef short v2s __attribute__((ext_vector_type(2)));
typedef unsigned short v2us __attribute__((ext_vector_type(2)));

struct TiledParams {
    const int8_t* src;  // owned row 0 of the source buffer
    int8_t* dst;        // owned row 0 of the destination buffer
    long long pitch;
    int rows, nchunks;           // owned rows; ceil(cols / 16) (the last chunk may be ragged)
    int cols;
    int q_shift;                 // first octet of tile column 0 (periodic lattices of ragged width: keeps the ragged octet out of every halo)
    int tile_h;                  // tile height of this launch (even; the template H is the default and the LDS budget)
    int flex_ty;                 // > 0: the rows [r_begin, r_end) are cut into flex_ty tile rows of (nearly) equal even heights
                                 // <= tile_h instead of rows of tile_h each (tile-resident runs of lattices of any height)
    int r_begin, r_end;          // rows this launch computes: [0, rows) or, for a slab that will sweep again before its
                                 // next ghost refresh, [-ext, rows + ext) so that its own halo stays exact
    long long row0, total_rows;  // global row of owned row 0; global lattice height
    int wrap_rows, ghost;        // source rows wrap inside the buffer, or come from `ghost` ghost rows
    int k;                       // sweeps in this launch
    int tiles_x;
    int ty_first, ty_stride;     // tile row of block b: ty_first + (b / tiles_x) * ty_stride
    uint32_t k0, k1, sweep0, tag_hi, tag_lo;
    uint32_t tblH0, tblH1, tblL0, tblL1;  // (min(thr >> 16, 65535) ^ 0x8000) for up = 0..4, split into byte tables
    uint32_t t3H0, t3H1, t3L0, t3L1;      // open lattices: the same for degree 3 (entries 0..3) and degree 2 (entries 4..6)
    int open;                             // open boundary: sites outside the lattice count as 0 "up" and lower the degree
    uint64_t thr[25];                     // full thresholds, [deg * 5 + up], for the tie path
};

// tile row ty of a launch: rows [row_off, row_off + H) of the launch's range
static __host__ __device__ __forceinline__ void tile_rows(const TiledParams& p, int ty, int& row_off, int& H) {
    H = p.tile_h;
    row_off = ty * p.tile_h;
    if (p.flex_ty > 0) {
        const long long half = (p.r_end - p.r_begin + 1) / 2;  // (an open lattice of odd height: the last tile row ends one row past it)
        row_off = 2 * (int)(ty * half / p.flex_ty);
        H = 2 * (int)((ty + 1) * half / p.flex_ty) - row_off;
    }
}
// global row of tile row 0 of that tile in a launch of k sweeps (wrapped on a periodic lattice), and whether the tile's window of
// H + 4k rows holds the lattice's wrap row (row total_rows - 1 followed by row 0; never on an open lattice)
static __host__ __device__ __forceinline__ bool tile_holds_wrap(const TiledParams& p, int ty, int k, long long& rg0) {
    int H, row_off;
    tile_rows(p, ty, row_off, H);
    rg0 = p.row0 + p.r_begin + row_off - 2 * k;
    if (p.open) return false;
    rg0 %= p.total_rows;
    if (rg0 < 0) rg0 += p.total_rows;
    return rg0 + H + 4 * k > p.total_rows;
}
// A lattice whose height is a power of two takes the wrap in the Philox head (philox_vk) at no cost
static __host__ __device__ __forceinline__ bool wrap_by_mask(const TiledParams& p) { return (p.total_rows & (p.total_rows - 1)) == 0; }

static __device__ __forceinline__ uint32_t perm(uint32_t s0, uint32_t s1, uint32_t sel) {
    return __builtin_amdgcn_perm(s0, s1, sel);
}
static __device__ __forceinline__ uint32_t subsat16(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(v2s, a), __builtin_bit_cast(v2s, b)));
}
static __device__ __forceinline__ uint32_t minu16(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(v2us, a), __builtin_bit_cast(v2us, b)));
}

// exact resolution of the (rare) fields whose top 16 bits tie with the threshold: d fields that are 0.
// Cold path (probability 2^-16 per site): kept out of line and register-to-register (no arrays by address).
template <uint32_t CSHIFT = 0>
static __device__ __noinline__ u32x4 resolve_ties(u32x4 d, u32x4 w, uint32_t cnt_lo, uint32_t cnt_hi, const uint64_t* s_thr,
                                                  uint32_t cq, uint32_t Rg, uint32_t hs, uint32_t tag_lo, uint32_t k0,
                                                  uint32_t k1, uint32_t edge = 0) {
    // edge (open lattices): bit 0 = the row is the lattice's top or bottom row, bit 1 = site 0 of the octet is in the
    // lattice's first column, bit 2 = site (edge >> 4) is in its last column; degree = 4 minus the missing neighbours
    // CSHIFT: the counts arrive scaled by 1 << CSHIFT (3 with the quad table, see pair_thresholds)
    const u32x4 l = tsu_philox(cq, Rg, hs, tag_lo, k0, k1);
#define TSU_FIX(DW, WW, LW, CNT, B0, M0)                                                                        \
    _Pragma("unroll") for (int hlf = 0; hlf < 2; ++hlf) {                                                       \
        const uint32_t sh = 16u * hlf;                                                                          \
        if (((DW >> sh) & 0xFFFFu) == 0) {                                                                      \
            const uint32_t c = ((CNT >> (8 * (B0 + hlf))) & 0xFFu) >> CSHIFT;                                   \
            const uint32_t m = M0 + hlf;                                                                        \
            const uint32_t deg = 4u - (edge & 1u) - ((m == 0 && (edge & 2u)) ? 1u : 0u) - ((m == (edge >> 4) && (edge & 4u)) ? 1u : 0u); \
            const uint64_t u = ((uint64_t)(((WW >> sh) & 0xFFFFu) ^ 0x8000u) << 16) | ((LW >> sh) & 0xFFFFu);   \
            const uint32_t f = (u < s_thr[deg * 5 + c]) ? 0x8000u : 0x0001u; /* negative field = accept */      \
            DW = (DW & ~(0xFFFFu << sh)) | (f << sh);                                                           \
        }                                                                                                       \
    }
    TSU_FIX(d.x, w.x, l.x, cnt_lo, 0, 0)
    TSU_FIX(d.y, w.y, l.y, cnt_lo, 2, 2)
    TSU_FIX(d.z, w.z, l.z, cnt_hi, 0, 4)
    TSU_FIX(d.w, w.w, l.w, cnt_hi, 2, 6)
#undef TSU_FIX
    return d;
}

// ================================================================== inner loop
// The half-sweep body is organised for instruction count and ILP:
//   * a thread owns ONE octet column for the whole kernel (global chunk index fixed, no div/mod in the loop) and
//     walks down the rows in pairs (r, r+1): the two rows share two of their three neighbour-row reads, and their
//     two Philox blocks are independent dependency chains that the scheduler interleaves;
//   * the ten round keys live in VGPRs (a v_xor with an SGPR operand issues at half the rate of a VGPR-only one);
//   * one tie test covers both rows.
struct PhiloxKeys {
    uint32_t a[10], b[10];
};

static __device__ __forceinline__ PhiloxKeys make_keys(uint32_t k0, uint32_t k1) {
    PhiloxKeys K;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint32_t x = k0 + (uint32_t)r * TSU_PHILOX_W0, y = k1 + (uint32_t)r * TSU_PHILOX_W1;
        if (r > 0) asm volatile("v_mov_b32 %0, %1" : "=v"(x) : "s"(x));  // opaque: keep the keys in vector registers (a[0]: see philox_y0)
        asm volatile("v_mov_b32 %0, %1" : "=v"(y) : "s"(y));
        K.a[r] = x;
        K.b[r] = y;
    }
    return K;
}

// (a & b) ^ c in one v_bitop3_b32 (truth table 0x6A)
static __device__ __forceinline__ uint32_t and_xor(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x6A); }

// The row enters the block in round 0 alone, as n0 = hi(M1 hs) ^ row ^ key: y0 = hi(M1 hs) ^ key is uniform per half-sweep
// (philox_y0) and the head is (row & rmask) ^ y0 -- the same single instruction as the XOR3 it replaces.  With
// rmask = total_rows - 1 on a lattice whose height is a power of two the periodic row wrap costs nothing: the caller's row
// counter runs on past the last row.  Everyone else passes all ones.  K.a[0] is not used: it lives in y0.
static __device__ __forceinline__ uint32_t philox_y0(uint32_t hs, uint32_t k0) {
    uint32_t y = (uint32_t)(((uint64_t)TSU_PHILOX_M1 * hs) >> 32) ^ k0;
    asm volatile("v_mov_b32 %0, %1" : "=v"(y) : "s"(y));  // a vector register, like the round keys (see PhiloxKeys)
    return y;
}

static __device__ __forceinline__ u32x4 philox_vk(uint32_t c0, uint32_t row, uint32_t rmask, uint32_t y0, uint32_t c2, uint32_t c3,
                                                  const PhiloxKeys& K) {
    uint32_t c1;
    {
        const uint64_t p0 = (uint64_t)TSU_PHILOX_M0 * c0;
        const uint64_t p1 = (uint64_t)TSU_PHILOX_M1 * c2;
        const uint32_t n0 = and_xor(row, rmask, y0);
        const uint32_t n2 = tsu_xor3((uint32_t)(p0 >> 32), c3, K.b[0]);
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
    }
#pragma unroll
    for (int r = 1; r < 10; ++r) {
        uint64_t p0 = (uint64_t)TSU_PHILOX_M0 * c0;
        uint64_t p1 = (uint64_t)TSU_PHILOX_M1 * c2;
        uint32_t n0 = tsu_xor3((uint32_t)(p1 >> 32), c1, K.a[r]);
        uint32_t n2 = tsu_xor3((uint32_t)(p0 >> 32), c3, K.b[r]);
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
    }
    return u32x4{c0, c1, c2, c3};
}

#define TSU_LDS __attribute__((address_space(3)))
static __device__ __forceinline__ uint32_t lds_addr(const void* p) { return (uint32_t)(uintptr_t)(const TSU_LDS char*)p; }
template <typename T>
static __device__ __forceinline__ T lds_ld(uint32_t a) { return *(const TSU_LDS T*)(uintptr_t)a; }
template <typename T>
static __device__ __forceinline__ void lds_st(uint32_t a, T v) { *(TSU_LDS T*)(uintptr_t)a = v; }

struct Rows2Ctx {
    const uint64_t* s_thr;
    int total_rows;
    int rg_tile0, wrap_tr;  // global row of tile row 0 (wrapped on a periodic lattice); EDGE tiles: the tile row whose global row is 0 again
    uint32_t rmask;         // total_rows - 1 where the Philox head takes the row wrap (see philox_vk and tile_body), else all ones
    uint32_t tag_hi, tag_lo, k0, k1;
    uint32_t tbl2;                        // periodic lattices: LDS byte address of the pair table (see pair_thresholds)
    uint32_t tblH0, tblH1, tblL0, tblL1;  // open lattices: the degree-4 byte tables (see compare_octet_open)
    uint32_t t3H0, t3H1, t3L0, t3L1;      // open lattices: degree 3 / degree 2 byte tables
    int last_row;                     // open lattices: global index of the lattice's bottom row
    bool lft, rgt;                    // open lattices: this thread's octet holds the lattice's first / last column
    uint32_t r_par, r_slot;           // open lattices: column parity of the last column and its site within the octet
    uint32_t rm_lo, rm_hi;            // 0xFF at that site's byte
    uint64_t vm_e, vm_o;              // open lattices: 0x01 for the even / odd columns of this octet that exist (byte planes)
    uint32_t nvm_e, nvm_o;            // the same in the nibble layout (nibble planes)
    int sh_next, sh_prev;             // periodic lattices of ragged width (SEAM): where the wrap meets this octet, see pair_step
};

// thresholds for the 8 sites of one octet given their up-counts, compared with one Philox block: d < 0 = accept
static __device__ __forceinline__ u32x4 compare_octet(const u32x4& w, uint32_t cnt_lo, uint32_t cnt_hi, uint32_t tH0,
                                                      uint32_t tH1, uint32_t tL0, uint32_t tL1) {
    const uint32_t Hl = perm(tH1, tH0, cnt_lo), Ll = perm(tL1, tL0, cnt_lo);
    const uint32_t Hh = perm(tH1, tH0, cnt_hi), Lh = perm(tL1, tL0, cnt_hi);
    u32x4 d;
    d.x = subsat16(w.x, perm(Hl, Ll, 0x05010400u));
    d.y = subsat16(w.y, perm(Hl, Ll, 0x07030602u));
    d.z = subsat16(w.z, perm(Hh, Lh, 0x05010400u));
    d.w = subsat16(w.w, perm(Hh, Lh, 0x07030602u));
    return d;
}

// The periodic tile kernels make the same compare without a v_perm.  The 16-bit thresholds of the site pair (j, j + 1) depend on
// the pair's two counts alone, 25 combinations, and w.x .. w.w hold such pairs: tbl2 (LDS, 25 dwords, built per tile in tile_body)
// holds t16(c0) | t16(c1) << 16 at dword c0 + 5 c1, already in the layout of a w word, and one v_dot4_u32_u8 with the byte weights
// (4, 20, 0, 0) or (0, 0, 4, 20) turns the four byte counts of a dword into the byte offset of sites (0, 1) or (2, 3).  The table
// sits at a compile-time LDS address, so the offset is the whole VGPR address and the base the instruction's offset field.  Per
// octet 4 v_dot4 + 4 ds_read_b32 for 8 v_perm; 25 consecutive dwords are 25 banks and equal addresses broadcast.
// (profiles/k1_pair_table_microbench.txt, k1_pair_table_ab.txt)
struct PairCounts {
    uint32_t c0l, c0h, c1l, c1h;  // up-counts of the pair's two octets, a byte per site: sites 0..3 and 4..7 of row a, of row b
};
struct PairThr {
    uint32_t t[8];  // threshold words of row a's octet (against w.x .. w.w), then of row b's
};
// QUAD (byte planes whose tile leaves the LDS for it, see tile_body): one look-up serves the four sites of a count dword.  Entry
// i = c0 + 5 c1 + 25 c2 + 125 c3 of tbl4 (625 x 8 bytes) holds t16(c0) | t16(c1) << 16 | t16(c2) << 32 | t16(c3) << 48, two
// consecutive w words.  The byte offset 8 i must come out of one v_dot4 and 8 x 125 is no byte weight, so the colour planes of
// these kernels hold their up-flags as 8 instead of 1: the counts arrive scaled by 8 (a byte is at most 32, nothing carries) and
// the weights are (1, 5, 25, 125).  Per pair 4 v_dot4 + 4 ds_read_b64 for 8 + 8.  Scattered 8-byte reads over 5 KB do meet bank
// conflicts, which lanes on neighbouring octets of an ordered lattice mostly avoid (profiles/k1_quad_table_microbench.txt).
constexpr uint32_t QUAD_FLAG = 8u, QUAD_SHIFT = 3u;
// issues the table reads of a pair; pair_step puts them in front of the second Philox block, which hides their latency
template <bool QUAD>
static __device__ __forceinline__ PairThr pair_thresholds(const PairCounts& n, uint32_t tbl2) {
    constexpr uint32_t W01 = 0x00001404u, W23 = 0x14040000u, WQ = 0x7D190501u;
    const uint32_t cnt[4] = {n.c0l, n.c0h, n.c1l, n.c1h};
    if constexpr (QUAD) {
        uint32_t off4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) off4[j] = __builtin_amdgcn_udot4(cnt[j], WQ, 0u, false);
        PairThr T;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t e = lds_ld<uint64_t>(tbl2 + off4[j]);
            T.t[2 * j] = (uint32_t)e;
            T.t[2 * j + 1] = (uint32_t)(e >> 32);
        }
        return T;
    }
    uint32_t off[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        off[2 * j] = __builtin_amdgcn_udot4(cnt[j], W01, 0u, false);
        off[2 * j + 1] = __builtin_amdgcn_udot4(cnt[j], W23, 0u, false);
    }
    PairThr T;
#pragma unroll
    for (int j = 0; j < 8; ++j) T.t[j] = lds_ld<uint32_t>(tbl2 + off[j]);
    return T;
}
static __device__ __forceinline__ u32x4 compare_octet_thr(const u32x4& w, const uint32_t* t) {
    return u32x4{subsat16(w.x, t[0]), subsat16(w.y, t[1]), subsat16(w.z, t[2]), subsat16(w.w, t[3])};
}

// Open lattices: as compare_octet, then the sites with fewer than four neighbours take their thresholds from the
// degree-3 / degree-2 table instead (row_edge: the whole row is the lattice's top or bottom row; l0: site 0 of the octet
// sits in the lattice's first column; r7: site c.r_slot sits in its last column -- site 7 unless the width is ragged).  Only executed by waves that hold such a site.
static __device__ __forceinline__ u32x4 compare_octet_open(const u32x4& w, uint32_t cnt_lo, uint32_t cnt_hi, const Rows2Ctx& c,
                                                           bool row_edge, bool l0, bool r7) {
    uint32_t Hl = perm(c.tblH1, c.tblH0, cnt_lo), Ll = perm(c.tblL1, c.tblL0, cnt_lo);
    uint32_t Hh = perm(c.tblH1, c.tblH0, cnt_hi), Lh = perm(c.tblL1, c.tblL0, cnt_hi);
    if (row_edge | l0 | r7) {
        // entries 0..3 = degree 3, 4..6 = degree 2 (a corner: edge row and edge column)
        const uint32_t rl = r7 ? c.rm_lo : 0u, rh = r7 ? c.rm_hi : 0u;
        const uint32_t il = cnt_lo + ((row_edge && l0) ? 0x00000004u : 0u) + (row_edge ? (rl & 0x04040404u) : 0u);
        const uint32_t ih = cnt_hi + (row_edge ? (rh & 0x04040404u) : 0u);
        const uint32_t ml = row_edge ? 0xFFFFFFFFu : ((l0 ? 0x000000FFu : 0u) | rl), mh = row_edge ? 0xFFFFFFFFu : rh;
        Hl = (Hl & ~ml) | (perm(c.t3H1, c.t3H0, il) & ml);
        Ll = (Ll & ~ml) | (perm(c.t3L1, c.t3L0, il) & ml);
        Hh = (Hh & ~mh) | (perm(c.t3H1, c.t3H0, ih) & mh);
        Lh = (Lh & ~mh) | (perm(c.t3L1, c.t3L0, ih) & mh);
    }
    u32x4 d;
    d.x = subsat16(w.x, perm(Hl, Ll, 0x05010400u));
    d.y = subsat16(w.y, perm(Hl, Ll, 0x07030602u));
    d.z = subsat16(w.z, perm(Hh, Lh, 0x05010400u));
    d.w = subsat16(w.w, perm(Hh, Lh, 0x07030602u));
    return d;
}

static __device__ __forceinline__ bool has_zero_field(const u32x4& d) {
    const uint32_t mn = minu16(minu16(d.x, d.y), minu16(d.z, d.w));
    return ((mn & 0xFFFFu) == 0) | ((mn >> 16) == 0);
}

template <bool QUAD = false>
static __device__ __forceinline__ uint64_t pack_flags(const u32x4& d) {
    // v_perm_b32 selectors 8..11 replicate the sign bit of the four 16-bit fields of {S0,S1} (bits 15, 31, 47, 63)
    // into a whole byte: one instruction turns the four "accept" signs into 0x00 / 0xFF bytes
    constexpr uint32_t FLM = (QUAD ? QUAD_FLAG : 1u) * 0x01010101u;
    const uint32_t nlo = perm(d.y, d.x, 0x0B0A0908u) & FLM;
    const uint32_t nhi = perm(d.w, d.z, 0x0B0A0908u) & FLM;
    return (uint64_t)nlo | ((uint64_t)nhi << 32);
}

// EDGE tiles: global rows of the pair at tile rows (tr, tr + 1).  The lattice's last row falls at ONE tile row (wrap_tr), so a
// wave's lanes (a few consecutive row lanes: tile rows tr_wave .. tr_wave + SPAN) lie on one side of it in all but one
// wave-iteration per half-sweep: the offset is a scalar select and the per-lane compares run in that one iteration only.
// The wave carries to_wrap = wrap_tr - tr_wave, counted down from pair to pair, so that both questions are one scalar
// compare each: "past the wrap" is to_wrap <= 0, "this iteration straddles it" is 0 < to_wrap <= SPAN, i.e.
// (unsigned)(to_wrap - 1) < SPAN -- 5 scalar instructions per pair where comparing tr_wave with wrap_tr twice and combining
// the two conditions took 10, on a dependent chain in front of the branch.  The edge tiles set every tile's pace (each
// generation's strips wait for them: profiles/resident_exchange_parent_timeline.txt), so what they lose all 256 tiles lose.
// (Tried instead: the wrapped row itself carried per lane, a subtract and an unsigned minimum per step and per row, no scalar
// work and no branch: as good on byte planes, 2.5 % slower on the nibble planes of 8192^2: profiles/resident_exchange_ab.txt.)
template <int NO>
static __device__ __forceinline__ void edge_rows(const Rows2Ctx& c, int to_wrap, int tr, int& rga, int& rgb) {
    constexpr int SPAN = 2 * ((NO - 1 + 63) / NO) + 1;  // tile rows below the first lane's that a wave's 64 lanes can reach
    const int s_off = to_wrap > 0 ? c.rg_tile0 : c.rg_tile0 - c.total_rows;
    rga = tr + s_off;
    rgb = rga + 1;
    if (__builtin_expect((uint32_t)(to_wrap - 1) < (uint32_t)SPAN, 0)) {  // wave-uniform
        rga = tr + c.rg_tile0;
        asm volatile("" : "+v"(rga));  // a real branch: as selects this would cost every iteration 9 instructions
        rgb = rga + 1;
        if (rga >= c.total_rows) rga -= c.total_rows;
        if (rgb >= c.total_rows) rgb -= c.total_rows;
    }
}

// ---- LDS layout of a tile and the pair loop's addressing
// The two colour planes are interleaved row by row: tile row r holds its NO octets of plane 0 and then its NO octets of
// plane 1, so a row is 2 NO octets and the distance between the planes is NO octets -- compile-time constants whatever the
// tile's height.  The pair loop keeps ONE address, the LDS byte address of (row tr - 1, its octet, source plane), and
// reaches the four rows it reads, the two side octets and the two octets it writes through the offset field of the DS
// instructions.  "Octet -1" and "octet NO" of a row are the last / first octet of the other plane's row next to it (for
// plane 0 of row 0: the guard octet, for plane 1 of the last row: the spare row): 0/1 flags that, like every neighbour beyond
// the tile, only feed the far side of a halo octet.  They lie in the plane that the half-sweep WRITES: the threads of octets 0 and
// NO - 1 read them while another wave may be storing them, without synchronisation.  Either value is a 0/1 flag and the sites
// it reaches never count, so results do not depend on it -- but the contents of the halo octets' far side (columns that a
// tile computes along and discards) are not deterministic from run to run.  Nothing may rely on them: compare or dump interiors.
// In front of the guard octet: the pair table of the periodic compare, 25 dwords rounded up to whole octets so that the planes keep
// their 8-byte alignment.  The tile kernels have no static LDS, so their dynamic LDS, and with it the table, starts at LDS address 0:
// a constant that the table reads carry in their offset field (through `lds` it would be a register and cost an add per read).
// A static __shared__ variable in a tile kernel would move the planes onto the table: every K1 parity test then fails.
constexpr int TBL2_OCTETS = 13;
constexpr int TBL4_OCTETS = 625;  // the quad table (see pair_thresholds) in its place
constexpr uint32_t TBL2_LDS_ADDR = 0;

// every indexer of the colour planes outside the pair loop: octet o of tile row r of plane pl
template <typename E, int NO>
struct TilePlanes {
    E* base;  // plane 0, row 0, octet 0
    __device__ __forceinline__ E& at(int pl, int r, int o) const { return base[(2 * r + pl) * NO + o]; }
};

// One pair of rows (tr, tr + 1) of one octet column; a = LDS byte address of (row tr - 1, this octet, source plane).
// KAPPA = colour of the half-sweep (the destination plane; the source is the other one)
// P0 = column parity of the updated colour in row tr (and 1-P0 in the row below it); it is the same for every half-sweep of
// a tile: the first row of half-sweep hsi is tile row 1 + hsi and its colour hsi & 1, and their sum is always odd
template <int NO, int KAPPA, int P0, bool EDGE, bool OPEN, bool SEAM, bool QUAD>
static __device__ __forceinline__ void pair_step(const Rows2Ctx& c, const PhiloxKeys& K, uint32_t hs, uint32_t y0, uint32_t a, int rg, int to_wrap,
                                                 uint32_t cq) {
    constexpr int RS = 2 * NO * 8;                    // row stride
    constexpr int DO = (KAPPA ? NO : -NO) * 8;        // source plane -> destination plane
    // issue the six LDS reads and run the Philox blocks (which do not depend on them) while they are in flight
    const uint64_t R0 = lds_ld<uint64_t>(a), R1 = lds_ld<uint64_t>(a + RS);
    const uint64_t R2 = lds_ld<uint64_t>(a + 2 * RS), R3 = lds_ld<uint64_t>(a + 3 * RS);
    // side octets: the last site of the previous octet (the top byte of its high dword) or the first site of the next one.  One of
    // the two reads is volatile so that they stay two ds_read_b32 with 16-bit offset fields: paired into a ds_read2_b32, whose
    // offset fields are 8 bits of dwords, they would need a second base register for NO = 34, i.e. an add per iteration.
    // (This steers the compiler's load pairing, which skips volatile accesses; results do not depend on it.  Whether it still
    // holds after a compiler change shows in tools/k1_loop_counts.py: the plain byte loop then has 6 v_add_u32 instead of 5.
    // Reading the one byte that is used, ds_read_u8, also avoids the pairing but cost a v_and in the EDGE loops.)
    const uint32_t A0 = SEAM ? 0u : (P0 ? lds_ld<volatile uint32_t>(a + RS + 8) : lds_ld<uint32_t>(a + RS - 4));
    const uint32_t A1 = SEAM ? 0u : (P0 ? lds_ld<uint32_t>(a + 2 * RS - 4) : lds_ld<volatile uint32_t>(a + 2 * RS + 8));
    // SEAM (a periodic lattice whose width is not a multiple of 16, workgroups whose window holds the wrap): the last
    // octet of a row has only v sites per colour, so the site after its last one is site 0 of octet 0, and the site
    // before site 0 of octet 0 is that last one: the whole neighbouring octet is read and the one byte that crosses
    // over is taken from / put at position v - 1 instead of 7 (sh_next / sh_prev; 56 for every other octet)
    const uint64_t Na = SEAM ? lds_ld<uint64_t>(a + RS + (P0 ? 8 : -8)) : 0ull;
    const uint64_t Nb = SEAM ? lds_ld<uint64_t>(a + 2 * RS + (P0 ? -8 : 8)) : 0ull;
    __builtin_amdgcn_sched_barrier(0);  // the reads stay above the Philox blocks
    int rga = rg, rgb = rg + 1;
    if (EDGE) edge_rows<NO>(c, to_wrap, rg, rga, rgb);
    // Periodic lattices take the counts and issue the eight threshold reads between the two Philox blocks (by then the plane
    // reads have landed), so that the table's latency passes under the second block; open lattices, which compare through
    // v_perm tables in registers, consume the planes below both blocks
    constexpr bool EARLY = !OPEN;
    auto counts = [&]() -> PairCounts {
        const uint32_t C0l = (uint32_t)R1, C0h = (uint32_t)(R1 >> 32), C1l = (uint32_t)R2, C1h = (uint32_t)(R2 >> 32);
        // horizontal neighbours: compact bytes (j, j+1) when the parity is 1, (j-1, j) when it is 0
        uint32_t S0l = P0 ? __builtin_amdgcn_alignbyte(C0h, C0l, 1) : __builtin_amdgcn_alignbyte(C0l, A0, 3);
        uint32_t S0h = P0 ? __builtin_amdgcn_alignbyte(A0, C0h, 1) : __builtin_amdgcn_alignbyte(C0h, C0l, 3);
        uint32_t S1l = P0 ? __builtin_amdgcn_alignbyte(C1l, A1, 3) : __builtin_amdgcn_alignbyte(C1h, C1l, 1);
        uint32_t S1h = P0 ? __builtin_amdgcn_alignbyte(C1h, C1l, 3) : __builtin_amdgcn_alignbyte(A1, C1h, 1);
        if (SEAM) {
            const uint64_t nxa = (Na & 0xFFull) << c.sh_next, pva = (Na >> c.sh_prev) & 0xFFull;
            const uint64_t nxb = (Nb & 0xFFull) << c.sh_next, pvb = (Nb >> c.sh_prev) & 0xFFull;
            const uint64_t Sa = P0 ? ((R1 >> 8) | nxa) : ((R1 << 8) | pva);
            const uint64_t Sb = P0 ? ((R2 << 8) | pvb) : ((R2 >> 8) | nxb);
            S0l = (uint32_t)Sa; S0h = (uint32_t)(Sa >> 32);
            S1l = (uint32_t)Sb; S1h = (uint32_t)(Sb >> 32);
        }
        // R1 + R2 is shared by both rows' vertical+centre sums
        const uint32_t ml = C0l + C1l, mh = C0h + C1h;
        return PairCounts{(uint32_t)R0 + ml + S0l, (uint32_t)(R0 >> 32) + mh + S0h, (uint32_t)R3 + ml + S1l, (uint32_t)(R3 >> 32) + mh + S1h};
    };
    PairCounts n;
    PairThr T;
    const u32x4 w0 = philox_vk(cq, (uint32_t)rga, c.rmask, y0, hs, c.tag_hi, K);
    if constexpr (EARLY) {
        __builtin_amdgcn_sched_barrier(0);
        n = counts();
        T = pair_thresholds<QUAD>(n, c.tbl2);
        __builtin_amdgcn_sched_barrier(0);
    }
    const u32x4 w1 = philox_vk(cq, (uint32_t)rgb, c.rmask, y0, hs, c.tag_hi, K);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (!EARLY) n = counts();
    const uint32_t cnt0l = n.c0l, cnt0h = n.c0h, cnt1l = n.c1l, cnt1h = n.c1h;
    u32x4 d0, d1;
    uint32_t edge_a = 0, edge_b = 0;
    if (OPEN) {
        // row a updates the columns of parity P0, row b those of parity 1 - P0: the lattice's first column is site 0
        // of octet 0 for parity 0, its last column site r_slot of the last octet for parity r_par
        const bool ea = rga == 0 || rga == c.last_row, eb = rgb == 0 || rgb == c.last_row;
        const bool la = !P0 && c.lft, ra = c.rgt && c.r_par == (uint32_t)P0, lb = P0 && c.lft, rb = c.rgt && c.r_par != (uint32_t)P0;
        d0 = compare_octet_open(w0, cnt0l, cnt0h, c, ea, la, ra);
        d1 = compare_octet_open(w1, cnt1l, cnt1h, c, eb, lb, rb);
        edge_a = (ea ? 1u : 0u) | (la ? 2u : 0u) | (ra ? 4u : 0u) | (c.r_slot << 4);
        edge_b = (eb ? 1u : 0u) | (lb ? 2u : 0u) | (rb ? 4u : 0u) | (c.r_slot << 4);
    } else {
        d0 = compare_octet_thr(w0, T.t);
        d1 = compare_octet_thr(w1, T.t + 4);
    }
    const uint32_t mn = minu16(minu16(minu16(d0.x, d0.y), minu16(d0.z, d0.w)), minu16(minu16(d1.x, d1.y), minu16(d1.z, d1.w)));
    if (__builtin_expect(((mn & 0xFFFFu) == 0) | ((mn >> 16) == 0), 0)) {
        if (has_zero_field(d0)) d0 = resolve_ties<QUAD ? QUAD_SHIFT : 0u>(d0, w0, cnt0l, cnt0h, c.s_thr, cq, (uint32_t)rga & c.rmask, hs, c.tag_lo, c.k0, c.k1, edge_a);
        if (has_zero_field(d1)) d1 = resolve_ties<QUAD ? QUAD_SHIFT : 0u>(d1, w1, cnt1l, cnt1h, c.s_thr, cq, (uint32_t)rgb & c.rmask, hs, c.tag_lo, c.k0, c.k1, edge_b);
    }
    uint64_t n0 = pack_flags<QUAD>(d0), n1 = pack_flags<QUAD>(d1);
    if (OPEN) {  // what lies beyond the open edge stays empty (it is a neighbour of the edge sites in the next half-sweep)
        n0 = (rga < 0 || rga > c.last_row) ? 0 : (n0 & (P0 ? c.vm_o : c.vm_e));
        n1 = (rgb < 0 || rgb > c.last_row) ? 0 : (n1 & (P0 ? c.vm_e : c.vm_o));
    }
    if (SEAM) {  // the sites the last octet does not have stay empty
        n0 &= c.vm_e;
        n1 &= c.vm_e;
    }
    lds_st<uint64_t>(a + RS + DO, n0);
    lds_st<uint64_t>(a + 2 * RS + DO, n1);
}

// One half-sweep of one thread: the pairs at tile rows tr, tr + 2 RL, ... of its octet column.  Every thread of the workgroup
// has n or n + 1 of them: n iterations run under scalar loop control (no per-lane trip count), the last one under the lane
// mask `tail`, and a wave none of whose lanes has one skips it.
// a = LDS byte address of (row tr - 1, this octet, source plane) and rg = row number of tile row tr are the only per-lane
// induction variables (kept opaque so that the compiler neither re-derives them from the trip counter nor the trip counter
// from them); every other address is an immediate, see pair_step.
// EDGE (the tile's window crosses the lattice's last row): rg counts tile rows and the wrap is applied per wave, see edge_rows
template <int NO, int RL, int KAPPA, int P0, bool EDGE, bool OPEN, bool SEAM, bool QUAD>
static __device__ __forceinline__ void sweep_pairs(const Rows2Ctx& c, const PhiloxKeys& K, uint32_t hs, uint32_t y0, uint32_t a, int rg, int n, bool tail,
                                                   uint32_t cq) {
    int to_wrap = EDGE ? c.wrap_tr - __builtin_amdgcn_readfirstlane(rg) : 0;  // from the wave's first lane (lanes ascend in rows)
    bool live = true;  // the last of the n + 1 trips runs under the lane mask `tail`: one copy of the body, a wave without a lane skips it
#pragma unroll 1
    for (int i = n; i >= 0; --i) {
        if (i == 0) live = tail;
        asm volatile("" : "+v"(a), "+v"(rg));
        if (live) pair_step<NO, KAPPA, P0, EDGE, OPEN, SEAM, QUAD>(c, K, hs, y0, a, rg, to_wrap, cq);
        a += 2 * RL * 2 * NO * 8;
        rg += 2 * RL;
        to_wrap -= 2 * RL;
    }
}


// ================================================================== nibble planes (NIB)
// The same update with the colour planes kept at 4 bits per site instead of 8: an octet is ONE dword, site j < 4 in the
// low nibble of byte j, site j >= 4 in the high nibble of byte j - 4 (so that `x & 0x0F0F0F0F` and `(x >> 4) & 0x0F0F0F0F`
// are the byte-per-site halves the threshold look-up wants).  Neighbour counts (<= 4) are summed nibble-wise with plain
// dword adds -- half the adds of the byte form -- and only the count is widened to bytes.  Half the LDS per site: a
// 512 x 512 tile (+ halo) fits one CU, which makes 8192^2 tile-resident and halves the halo work of the big lattices.
// Periodic lattices whose width is a multiple of 16 only (no OPEN / SEAM forms).
static __device__ __forceinline__ uint32_t nib_shift_next(uint32_t X, uint32_t N) {
    // S_j = X_{j+1}; site 3 <- site 4 (high nibble of byte 0), site 7 <- site 0 of the next octet N
    const uint32_t hi = (N << 4) | __builtin_amdgcn_ubfe(X, 4u, 4u);
    return __builtin_amdgcn_alignbit(hi, X, 8);
}
static __device__ __forceinline__ uint32_t nib_shift_prev(uint32_t X, uint32_t M) {
    // S_j = X_{j-1}; site 4 <- site 3 (low nibble of byte 3), site 0 <- site 7 of the previous octet M
    const uint32_t w = ((X << 4) & 0x10000000u) | (M >> 4);
    return __builtin_amdgcn_alignbit(X, w, 24);
}
// SEAM (periodic width not a multiple of 16, see pair_step): the octet that crosses over sits at site v - 1 of the ragged
// last octet instead of site 7 -- bit position `pos` = 8 (j & 3) + 4 (j >> 2) of site j (28 for every other octet)
static __device__ __forceinline__ uint32_t nib_shift_next_seam(uint32_t X, uint32_t N, int pos) {
    return nib_shift_next(X, 0u) | ((N & 0xFu) << pos);  // (site v of a ragged octet is empty, so the slot is free)
}
static __device__ __forceinline__ uint32_t nib_shift_prev_seam(uint32_t X, uint32_t M, int pos) {
    const uint32_t w = ((X << 4) & 0x10000000u) | (((M >> pos) & 0xFu) << 24);
    return __builtin_amdgcn_alignbit(X, w, 24);
}
static __device__ __forceinline__ uint32_t nib_pack(const u32x4& d) {
    const uint64_t f = pack_flags(d);
    return (uint32_t)f | ((uint32_t)(f >> 32) << 4);
}

// pair_step on nibble planes: the same addressing with dword octets (every offset halves)
template <int NO, int KAPPA, int P0, bool EDGE, bool OPEN, bool SEAM>
static __device__ __forceinline__ void pair_step_nib(const Rows2Ctx& c, const PhiloxKeys& K, uint32_t hs, uint32_t y0, uint32_t a, int rg, int to_wrap,
                                                     uint32_t cq) {
    constexpr int RS = 2 * NO * 4;
    constexpr int DO = (KAPPA ? NO : -NO) * 4;
    const uint32_t R0 = lds_ld<uint32_t>(a), R1 = lds_ld<uint32_t>(a + RS);
    const uint32_t R2 = lds_ld<uint32_t>(a + 2 * RS), R3 = lds_ld<uint32_t>(a + 3 * RS);
    const uint32_t A0 = lds_ld<uint32_t>(a + RS + (P0 ? 4 : -4));      // row a: next octet if P0, else the previous one
    const uint32_t A1 = lds_ld<uint32_t>(a + 2 * RS + (P0 ? -4 : 4));  // row b: the other side
    __builtin_amdgcn_sched_barrier(0);
    int rga = rg, rgb = rg + 1;
    if (EDGE) edge_rows<NO>(c, to_wrap, rg, rga, rgb);
    constexpr bool EARLY = !OPEN;  // as in pair_step
    auto counts = [&]() -> PairCounts {
        const uint32_t Sa = SEAM ? (P0 ? nib_shift_next_seam(R1, A0, c.sh_next) : nib_shift_prev_seam(R1, A0, c.sh_prev))
                                 : (P0 ? nib_shift_next(R1, A0) : nib_shift_prev(R1, A0));
        const uint32_t Sb = SEAM ? (P0 ? nib_shift_prev_seam(R2, A1, c.sh_prev) : nib_shift_next_seam(R2, A1, c.sh_next))
                                 : (P0 ? nib_shift_prev(R2, A1) : nib_shift_next(R2, A1));
        const uint32_t mid = R1 + R2;  // shared by both rows' vertical + centre sums
        const uint32_t cnt0 = R0 + mid + Sa, cnt1 = R3 + mid + Sb;
        return PairCounts{cnt0 & 0x0F0F0F0Fu, (cnt0 >> 4) & 0x0F0F0F0Fu, cnt1 & 0x0F0F0F0Fu, (cnt1 >> 4) & 0x0F0F0F0Fu};
    };
    PairCounts n;
    PairThr T;
    const u32x4 w0 = philox_vk(cq, (uint32_t)rga, c.rmask, y0, hs, c.tag_hi, K);
    if constexpr (EARLY) {
        __builtin_amdgcn_sched_barrier(0);
        n = counts();
        T = pair_thresholds<false>(n, c.tbl2);
        __builtin_amdgcn_sched_barrier(0);
    }
    const u32x4 w1 = philox_vk(cq, (uint32_t)rgb, c.rmask, y0, hs, c.tag_hi, K);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (!EARLY) n = counts();
    const uint32_t cnt0l = n.c0l, cnt0h = n.c0h, cnt1l = n.c1l, cnt1h = n.c1h;
    u32x4 d0, d1;
    uint32_t edge_a = 0, edge_b = 0;
    if (OPEN) {  // as in pair_step: the counts are bytes by now, the degree-3 / degree-2 patches are the byte form's
        const bool ea = rga == 0 || rga == c.last_row, eb = rgb == 0 || rgb == c.last_row;
        const bool la = !P0 && c.lft, ra = c.rgt && c.r_par == (uint32_t)P0, lb = P0 && c.lft, rb = c.rgt && c.r_par != (uint32_t)P0;
        d0 = compare_octet_open(w0, cnt0l, cnt0h, c, ea, la, ra);
        d1 = compare_octet_open(w1, cnt1l, cnt1h, c, eb, lb, rb);
        edge_a = (ea ? 1u : 0u) | (la ? 2u : 0u) | (ra ? 4u : 0u) | (c.r_slot << 4);
        edge_b = (eb ? 1u : 0u) | (lb ? 2u : 0u) | (rb ? 4u : 0u) | (c.r_slot << 4);
    } else {
        d0 = compare_octet_thr(w0, T.t);
        d1 = compare_octet_thr(w1, T.t + 4);
    }
    const uint32_t mn = minu16(minu16(minu16(d0.x, d0.y), minu16(d0.z, d0.w)), minu16(minu16(d1.x, d1.y), minu16(d1.z, d1.w)));
    if (__builtin_expect(((mn & 0xFFFFu) == 0) | ((mn >> 16) == 0), 0)) {
        if (has_zero_field(d0)) d0 = resolve_ties(d0, w0, cnt0l, cnt0h, c.s_thr, cq, (uint32_t)rga & c.rmask, hs, c.tag_lo, c.k0, c.k1, edge_a);
        if (has_zero_field(d1)) d1 = resolve_ties(d1, w1, cnt1l, cnt1h, c.s_thr, cq, (uint32_t)rgb & c.rmask, hs, c.tag_lo, c.k0, c.k1, edge_b);
    }
    uint32_t n0 = nib_pack(d0), n1 = nib_pack(d1);
    if (OPEN) {  // what lies beyond the open edge stays empty (existing-site masks in the nibble layout)
        n0 = (rga < 0 || rga > c.last_row) ? 0u : (n0 & (P0 ? c.nvm_o : c.nvm_e));
        n1 = (rgb < 0 || rgb > c.last_row) ? 0u : (n1 & (P0 ? c.nvm_e : c.nvm_o));
    }
    if (SEAM) {  // the sites the last octet does not have stay empty
        n0 &= c.nvm_e;
        n1 &= c.nvm_e;
    }
    lds_st<uint32_t>(a + RS + DO, n0);
    lds_st<uint32_t>(a + 2 * RS + DO, n1);
}

template <int NO, int RL, int KAPPA, int P0, bool EDGE, bool OPEN = false, bool SEAM = false>
static __device__ __forceinline__ void sweep_pairs_nib(const Rows2Ctx& c, const PhiloxKeys& K, uint32_t hs, uint32_t y0, uint32_t a, int rg, int n, bool tail,
                                                       uint32_t cq) {
    int to_wrap = EDGE ? c.wrap_tr - __builtin_amdgcn_readfirstlane(rg) : 0;
    bool live = true;  // the last of the n + 1 trips runs under the lane mask `tail`: one copy of the body, a wave without a lane skips it
#pragma unroll 1
    for (int i = n; i >= 0; --i) {
        if (i == 0) live = tail;
        asm volatile("" : "+v"(a), "+v"(rg));
        if (live) pair_step_nib<NO, KAPPA, P0, EDGE, OPEN, SEAM>(c, K, hs, y0, a, rg, to_wrap, cq);
        a += 2 * RL * 2 * NO * 4;
        rg += 2 * RL;
        to_wrap -= 2 * RL;
    }
}

// Half-sweep hsi = 2 s + KAPPA of a generation on one tile of TR rows: rows [1 + hsi, TR - 2 - hsi] in pairs (TR is even),
// thread (al, octet) takes every RL-th pair from pair al on.  a_thr = LDS byte address of (row 2 al, the thread's octet, plane 0)
template <int NO, int RL, int KAPPA, int P0, bool EDGE, bool OPEN, bool SEAM, bool NIB, bool QUAD>
static __device__ __forceinline__ void half_sweep(const Rows2Ctx& c, const PhiloxKeys& K, int TR, uint32_t sweep, int s, uint32_t a_thr, int al,
                                                  uint32_t cq) {
    constexpr int ES = NIB ? 4 : 8;
    const int hsi = 2 * s + KAPPA;
    __syncthreads();
    if (al < RL) {
        const int npairs = (TR - 2 - 2 * hsi) / 2;
        const int n = __builtin_amdgcn_readfirstlane(npairs / RL);  // every thread has n pairs, row lanes [0, npairs - n RL) one more
        const bool tail = al < npairs - n * RL;
        const uint32_t a = a_thr + (uint32_t)(hsi * 2 * NO * ES + (KAPPA ? 0 : NO * ES));  // the source is the other colour's plane
        int rg;  // row number of the thread's first row, tile row 1 + hsi + 2 al: its tile row (EDGE) or its global row
        if (EDGE) {
            rg = 1 + hsi + 2 * al;
        } else {
            int rgf = c.rg_tile0 + 1 + hsi;
            if (!OPEN && rgf >= c.total_rows) rgf -= c.total_rows;  // (a window past the wrap row: only where c.rmask takes the wrap)
            rg = rgf + 2 * al;
        }
        const uint32_t hs = 2u * sweep + (uint32_t)KAPPA;
        const uint32_t y0 = philox_y0(hs, c.k0);
        if constexpr (NIB) sweep_pairs_nib<NO, RL, KAPPA, P0, EDGE, OPEN, SEAM>(c, K, hs, y0, a, rg, n, tail, cq);
        else sweep_pairs<NO, RL, KAPPA, P0, EDGE, OPEN, SEAM, QUAD>(c, K, hs, y0, a, rg, n, tail, cq);
    }
}

// the kg sweeps of one generation, two half-sweeps per trip: colour 0, then colour 1
template <int NO, int RL, int P0, bool EDGE, bool OPEN, bool SEAM, bool NIB, bool QUAD>
static __device__ __forceinline__ void sweep_generation(const Rows2Ctx& c, const PhiloxKeys& K, int TR, uint32_t sweep_g, int kg, uint32_t a_thr,
                                                        int al, uint32_t cq) {
#pragma unroll 1
    for (int s = 0; s < kg; ++s) {
        half_sweep<NO, RL, 0, P0, EDGE, OPEN, SEAM, NIB, QUAD>(c, K, TR, sweep_g + (uint32_t)s, s, a_thr, al, cq);
        half_sweep<NO, RL, 1, P0, EDGE, OPEN, SEAM, NIB, QUAD>(c, K, TR, sweep_g + (uint32_t)s, s, a_thr, al, cq);
    }
}

// one tile: HBM -> LDS planes, 2k half-sweeps, interior -> HBM (the other buffer)
// Tile-resident generations (RESIDENT): when every tile of the lattice has its own workgroup on the chip at the same
// time, a tile stays in LDS for many generations of k sweeps; after each generation it publishes the 2k interior rows
// at its top and bottom and its first and last interior octet column (the colour planes as they are, ~20 KB) to a
// global exchange buffer and refreshes its halo from its eight neighbours' strips, whose elements carry their
// generation number (no flags: see the exchange in tile_body).  The full-tile stage and store (87 + 64 KB per
// generation) and the launch gap happen once per call instead of once per generation.
// The strips travel through agent-scope relaxed atomic stores and loads (performed at the device's coherence point,
// past the per-CU L1 and the per-XCD L2, like dense_coop.hip's shared data), so no cache write-back / invalidate is
// needed: with release/acquire fences the publish step alone cost 5 us per generation.
static __device__ __forceinline__ void xst(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
static __device__ __forceinline__ uint64_t xld(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct ResidentParams {
    uint64_t* xbuf;  // [2 parities][tiles][XSTRIDE] exchange strips; every element carries its generation number (see tile_body)
    uint32_t gen0;   // number of the first generation this launch publishes (1 .. 16383, counted on from launch to launch)
    int* err;        // host-mapped: set if a bounded wait expired (results invalid)
    int n_gen, k_last, tiles_y;
    int wrap_y;      // tile rows wrap (whole periodic lattice); 0 for a slab: its outer tile rows have no neighbour there and
                     // live on the slab's deep ghost rows (the region that is still exact shrinks, as between exchanges),
                     // and for an open lattice: beyond the edge there is nothing, and nothing stays there
    int wrap_x;      // tile columns wrap (periodic); 0 for an open lattice
    long long* dbg;  // TSU_K1_VERBOSE=2: per tile, wall_clock64 ticks spent in [sweeps, publish, wait, fetch]
};

// QUAD: periodic byte planes with the 625-entry threshold table and up-flags stored as QUAD_FLAG (see pair_thresholds): the host
// takes this form where the larger table fits beside the tile that the 25-entry form was planned with
template <int HT, int WO, int THREADS, bool OPEN = false, bool RESIDENT = false, bool NIB = false, bool QUAD = false>
static __device__ __forceinline__ void tile_body(const TiledParams& p, const int8_t* __restrict__ src, int8_t* __restrict__ dst,
                                                 const int k, const uint32_t sweep0, const int tx, const int ty, uint64_t* lds,
                                                 const PhiloxKeys& K, const ResidentParams* R = nullptr) {
    constexpr int NO = WO + 2;
    constexpr int RLMAX = THREADS / NO;
    int H, row_off;
    tile_rows(p, ty, row_off, H);
    const int TR = H + 4 * k;
    // Row lanes: threads [0, RL*NO) sweep (thread = one octet column x every RL-th row pair); all threads load and
    // store.  What a half-sweep costs is the busiest SIMD's sum of wave-iterations: with every lane in use the last,
    // partial iteration occupies the fewest waves and those are consecutive, i.e. spread round-robin over the four
    // SIMDs (+5 % on 4096^2 against the smallest lane count that reaches the same iteration count).
    constexpr int RL = RLMAX;
    using E = typename std::conditional<NIB, uint32_t, uint64_t>::type;  // one octet of a colour plane
    // the pair table of the periodic compare (pair_thresholds) at the start of the workgroup's LDS, the guard octet behind it
    static_assert(!QUAD || (!OPEN && !NIB), "the quad table is for periodic byte planes");
    constexpr uint32_t FL = QUAD ? QUAD_FLAG : 1u;  // an up-flag of the colour planes
    uint64_t* const guard = lds + (QUAD ? TBL4_OCTETS : TBL2_OCTETS);
    // the colour planes, interleaved row by row (see TilePlanes): plane 0 of row 0 starts behind the guard octet
    const TilePlanes<E, NO> P{reinterpret_cast<E*>(guard + 1)};
    // one spare row behind the planes: "octet NO" of plane 1 of the last row is read there (rounded up to the uint64 grid)
    uint64_t* s_thr = reinterpret_cast<uint64_t*>((reinterpret_cast<uintptr_t>(P.base + 2 * TR * NO + NO + 1) + 7u) & ~(uintptr_t)7u);
    const int tid = threadIdx.x;
    if (tid < 25) s_thr[tid] = p.thr[tid];
    // the top 16 bits of the degree-4 thresholds, as pack_thresholds makes them for the byte tables
    auto t16 = [&](int up) {
        const uint64_t thi = p.thr[4 * 5 + up] >> 16;
        return (uint32_t)(thi > 65535u ? 65535u : thi) ^ 0x8000u;
    };
    if (!OPEN && !QUAD && tid < 25) reinterpret_cast<uint32_t*>(lds)[tid] = t16(tid % 5) | (t16(tid / 5) << 16);
    if constexpr (QUAD) {
        for (int i = tid; i < TBL4_OCTETS; i += THREADS) {
            const uint32_t lo = t16(i % 5) | (t16(i / 5 % 5) << 16), hi = t16(i / 25 % 5) | (t16(i / 125) << 16);
            lds[i] = (uint64_t)lo | ((uint64_t)hi << 32);
        }
        // "octet -1" of row 0 and "octet NO" of the last row (see TilePlanes) feed counts that nothing reads, but here a count is
        // part of an 8-byte LDS address: they hold flags like every other octet (the guard's low word is s_fail, 0 while sweeping)
        if (tid == 0) *guard = 0;
        if (tid <= NO) P.base[2 * TR * NO + tid] = 0;
    }

    const int q0 = tx * WO + p.q_shift, r0 = p.r_begin + row_off, Rb = r0 - 2 * k;

    // a thread owns one octet column (al = row lane, oct = column) in all three phases: no div/mod in any loop
    const int al = tid / NO, oct = tid - al * NO;
    int cqi = q0 - 1 + oct;
    // open lattice: octets outside the lattice hold no spins (flags 0); their (discarded) results still take a counter
    const bool col_out = OPEN && (cqi < 0 || cqi >= p.nchunks);
    if (!OPEN) {
        if (cqi < 0) cqi += p.nchunks;
        if (cqi >= p.nchunks) cqi -= p.nchunks;
        if (cqi >= p.nchunks) cqi -= p.nchunks;
    }
    const uint32_t cq = (uint32_t)cqi;
    // open lattices of ragged width: the columns of this thread's chunk that exist (all 16, fewer in the last chunk, none outside)
    int nv = p.cols - 16 * cqi;  // (cqi: the octet's own index in the lattice, wrapped for a periodic one)
    if (col_out) nv = 0;
    if (nv > 16) nv = 16;
    auto first_sites = [](int n) { return n >= 8 ? 0x0101010101010101ull : (((1ull << (8 * n)) - 1) & 0x0101010101010101ull); };
    const uint64_t vm_e = first_sites((nv + 1) >> 1) * FL, vm_o = first_sites(nv >> 1) * FL;

    if (al < RLMAX) {
        const int8_t* col = src + 16 * (long long)(OPEN ? (cqi < 0 ? 0 : (cqi >= p.nchunks ? p.nchunks - 1 : cqi)) : cqi);
        // four rows per step, all four 16-byte loads in flight before the first is converted: the stage is one
        // HBM latency per step, so fewer, wider steps
        constexpr int LB = 4;
        for (int tr0 = al; tr0 < TR; tr0 += LB * RLMAX) {
            uint4 v[LB];
#pragma unroll
            for (int b = 0; b < LB; ++b) {
                const int tr = tr0 + b * RLMAX;
                const int rl = Rb + (tr < TR ? tr : TR - 1);
                int srow;
                if (p.wrap_rows) srow = rl < 0 ? rl + p.rows : (rl >= p.rows ? rl - p.rows : rl);  // rows >= TR: one wrap
                else srow = rl < -p.ghost ? -p.ghost : (rl >= p.rows + p.ghost ? p.rows + p.ghost - 1 : rl);
                v[b] = *reinterpret_cast<const uint4*>(col + (long long)srow * p.pitch);
            }
#pragma unroll
            for (int b = 0; b < LB; ++b) {
                const int tr = tr0 + b * RLMAX;
                if (tr < TR) {
                    // de-interleave the two colours, then +1 (0x01) -> 1, -1 (0xFF) -> 0: bit 1 of the byte, inverted
                    const uint32_t e0 = perm(v[b].y, v[b].x, 0x06040200u), e1 = perm(v[b].w, v[b].z, 0x06040200u);
                    const uint32_t o0 = perm(v[b].y, v[b].x, 0x07050301u), o1 = perm(v[b].w, v[b].z, 0x07050301u);
                    // (QUAD: the flag is bit 3 of the byte)
                    auto up = [](uint32_t x) { return ~(QUAD ? x << 2 : x >> 1) & (FL * 0x01010101u); };
                    uint64_t ev = (uint64_t)up(e0) | ((uint64_t)up(e1) << 32);
                    uint64_t od = (uint64_t)up(o0) | ((uint64_t)up(o1) << 32);
                    if (OPEN) {
                        const long long grow = p.row0 + Rb + tr;
                        if (grow < 0 || grow >= p.total_rows) ev = od = 0;  // beyond the open edge: nothing there
                    }
                    if (OPEN || nv < 16) {  // the pad bytes of a ragged last chunk are 0, which would read as "up"
                        ev &= vm_e;
                        od &= vm_o;
                    }
                    const int gpar = (int)((p.row0 + Rb + tr) & 1);  // colour of the even columns of this row
                    if (NIB) {
                        P.at(gpar, tr, oct) = (E)((uint32_t)ev | ((uint32_t)(ev >> 32) << 4));
                        P.at(gpar ^ 1, tr, oct) = (E)((uint32_t)od | ((uint32_t)(od >> 32) << 4));
                    } else {
                        P.at(gpar, tr, oct) = (E)ev;
                        P.at(gpar ^ 1, tr, oct) = (E)od;
                    }
                }
            }
        }
    }

    // A window that holds the lattice's wrap row: where the height is a power of two the pair loop's row counter runs on past the
    // last row (up to rg0 + TR - 1 < 2 total_rows) and the Philox head masks it -- the plain loop; other heights take the EDGE loop,
    // whose tiles are 1-2 us per generation slower than the plain ones and set every tile's pace (profiles/k1_row_mask_ab.txt).
    // Open lattices do not wrap (rows beyond the edge are discarded, and may be negative: never masked).
    long long rg0;
    const bool holds_wrap = tile_holds_wrap(p, ty, k, rg0);
    const bool edge = holds_wrap && !wrap_by_mask(p);

    Rows2Ctx c;
    c.s_thr = s_thr;
    c.total_rows = (int)p.total_rows;
    c.rg_tile0 = (int)rg0;
    c.wrap_tr = (int)(p.total_rows - rg0);
    asm volatile("v_mov_b32 %0, %1" : "=v"(c.rmask) : "s"(holds_wrap && !edge ? (uint32_t)p.total_rows - 1u : 0xFFFFFFFFu));
    c.tag_hi = p.tag_hi; c.tag_lo = p.tag_lo; c.k0 = p.k0; c.k1 = p.k1;
    c.tbl2 = TBL2_LDS_ADDR;
    c.tblH0 = c.tblH1 = c.tblL0 = c.tblL1 = 0;
    c.t3H0 = p.t3H0; c.t3H1 = p.t3H1; c.t3L0 = p.t3L0; c.t3L1 = p.t3L1;
    c.last_row = (int)p.total_rows - 1;
    c.lft = OPEN && cqi == 0;
    c.rgt = OPEN && cqi == p.nchunks - 1;
    c.r_par = (uint32_t)(p.cols - 1) & 1u;
    c.r_slot = ((uint32_t)(p.cols - 1) & 15u) >> 1;
    c.rm_lo = c.r_slot < 4 ? 0xFFu << (8 * c.r_slot) : 0u;
    c.rm_hi = c.r_slot < 4 ? 0u : 0xFFu << (8 * (c.r_slot - 4));
    c.vm_e = NIB ? 0 : vm_e;  // (each form of the planes keeps only its own masks alive through the sweeps)
    c.vm_o = NIB ? 0 : vm_o;
    c.nvm_e = NIB ? ((uint32_t)vm_e | ((uint32_t)(vm_e >> 32) << 4)) : 0u;
    c.nvm_o = NIB ? ((uint32_t)vm_o | ((uint32_t)(vm_o >> 32) << 4)) : 0u;
    // periodic lattice of ragged width: v sites per colour in the last octet of a row (cols is even: the same for both)
    const int v_last = (p.cols >> 1) & 7;
    const bool ragged = !OPEN && v_last != 0;
    const int seam_site = v_last - 1;  // the site of the ragged octet that is followed by site 0 of octet 0
    const int seam_pos = NIB ? 8 * (seam_site & 3) + 4 * (seam_site >> 2) : 8 * seam_site, last_pos = NIB ? 28 : 56;
    c.sh_next = (ragged && cqi == p.nchunks - 1) ? seam_pos : last_pos;
    c.sh_prev = (ragged && cqi == 0) ? seam_pos : last_pos;
    // does this workgroup's window (octets q0 - 1 .. q0 + WO of the periodic extension) hold the ragged octet or octet 0?
    int w0 = (q0 - 1) % p.nchunks;
    if (w0 < 0) w0 += p.nchunks;
    const bool seam = ragged && (w0 == 0 || w0 + NO - 1 >= p.nchunks - 1);
    if constexpr (OPEN) {
        // the threshold byte tables live in VGPRs: v_perm_b32 may read only one SGPR, so SGPR tables cost a v_mov per use
        asm volatile("v_mov_b32 %0, %1" : "=v"(c.tblH0) : "s"(p.tblH0));
        asm volatile("v_mov_b32 %0, %1" : "=v"(c.tblH1) : "s"(p.tblH1));
        asm volatile("v_mov_b32 %0, %1" : "=v"(c.tblL0) : "s"(p.tblL0));
        asm volatile("v_mov_b32 %0, %1" : "=v"(c.tblL1) : "s"(p.tblL1));
    }

    const int n_gen = RESIDENT ? R->n_gen : 1;
    long long tl0 = 0, tl[4] = {0, 0, 0, 0};
    const bool timing = RESIDENT && R->dbg && tid == 0;
    if (timing) tl0 = wall_clock64();
#define RES_MARK(q)                         \
    if (timing) {                           \
        const long long now_ = wall_clock64(); \
        tl[q] += now_ - tl0;                \
        tl0 = now_;                         \
    }
    // RESIDENT: "a neighbour wait expired in this workgroup" -- kept in the guard octet in front of plane 0 (only ever read
    // as "octet -1" padding of row 0): a static __shared__ word would push a 160 KB workgroup past the CU's LDS
    volatile int& s_fail = *reinterpret_cast<volatile int*>(guard);
    if (RESIDENT && tid == 0) s_fail = 0;

    // ---- the strip exchange between generations (RESIDENT).  Only colour plane 1 travels: a generation starts with the
    // half-sweep of colour 0, which rewrites every colour-0 site of the tile (halo included) from colour 1 alone.
    // Layout of a tile's slot: TOP[n_tb] BOTTOM[n_tb] LEFT[n_lr] RIGHT[n_lr].
    // Every strip element (8 up-flags, one per byte) carries the 14-bit number of its generation in the spare bits 1..7
    // of its bytes 0 and 1, so a reader validates each element by itself: no "strips complete" flag, no wait for the
    // stores to be acknowledged before raising one, no wait for the flag before fetching -- the refresh is a single
    // round trip that is repeated only for the elements that were not there yet.  (A slot is rewritten every second
    // generation and neighbours are never more than one generation apart, so a stale element always carries another
    // number; the host clears the buffer when the numbering restarts or the strip layout changes.)
    // (nibble planes: an element is the octet's dword, the number sits above it in bits 32..45; QUAD: the flag is bit 3 of a byte
    // and the number takes bits 0..2 and 4..7 of bytes 0 and 1)
    // On byte planes the number stands once more in the element's other dword (bytes 4 and 5) and the reader compares both
    // copies: an element is accepted only whole, whatever the width and the atomicity of the load that fetched it.  (Nibble
    // planes keep it above the flag dword alone: with both copies 8192^2 measured 0.6 % slower, profiles/k1_strip_dma_ab.txt.)  (An exchange that fetches the strips with 16-byte LDS-direct loads under a first pass of the
    // next half-sweep was built on this and measured slower than this one: profiles/k1_strip_dma_notes.txt.)
    const int n_tb = 2 * k * WO, n_lr = H;  // elements of a top/bottom and of a left/right strip
    const int xstride = 2 * n_tb + 2 * p.tile_h;  // (tile rows of a flexible cut differ by two rows: one slot size for all)
    // The last tile column of a lattice whose width is not a multiple of the tile width holds wi < WO lattice octets: its last
    // interior octet is tile octet wi, its right halo tile octet wi + 1; what lies beyond is the lattice's periodic continuation
    // from the stage, computed along and never read by anything that counts (it decays like the far side of any halo octet).
    const int wi = (p.nchunks + p.q_shift - q0) < WO ? (p.nchunks + p.q_shift - q0) : WO;
    constexpr uint64_t TAG_MASK = NIB ? 0xFFFFFFFF00000000ull : (QUAD ? 0x0000F7F70000F7F7ull : 0x0000FEFE0000FEFEull);
    constexpr uint64_t FLAG_MASK = NIB ? 0x11111111ull : FL * 0x0101010101010101ull;
    auto strip_tag = [&](int gen) -> uint64_t {
        const uint32_t G = R->gen0 + (uint32_t)gen;
        if (NIB) return (uint64_t)G << 32;
        uint64_t t;
        if (QUAD) {
            auto beside_bit3 = [](uint32_t g7) { return (uint64_t)((g7 & 7u) | ((g7 >> 3) << 4)); };
            t = beside_bit3(G & 0x7Fu) | (beside_bit3((G >> 7) & 0x7Fu) << 8);
        } else {
            t = ((uint64_t)(G & 0x7Fu) << 1) | ((uint64_t)((G >> 7) & 0x7Fu) << 9);
        }
        return t | (t << 32);
    };
    // publish generation gen's boundary strips: its first / last 2k interior rows and first / last interior octet column
    auto publish = [&](int gen) {
        RES_MARK(0);
        const int ntiles = p.tiles_x * R->tiles_y, me = ty * p.tiles_x + tx;
        uint64_t* mine = R->xbuf + ((size_t)(gen & 1) * ntiles + me) * xstride;
        const uint64_t tag = strip_tag(gen);
        for (int i = tid; i < n_tb; i += THREADS) {
            const int r = i / WO, o = i - r * WO;
            xst(mine + i, (uint64_t)P.at(1, 2 * k + r, 1 + o) | tag);     // TOP: first 2k interior rows
            xst(mine + n_tb + i, (uint64_t)P.at(1, H + r, 1 + o) | tag);  // BOTTOM: last 2k interior rows
        }
        for (int i = tid; i < n_lr; i += THREADS) {
            xst(mine + 2 * n_tb + i, (uint64_t)P.at(1, 2 * k + i, 1) | tag);          // LEFT: first interior octet
            xst(mine + 2 * n_tb + n_lr + i, (uint64_t)P.at(1, 2 * k + i, wi) | tag);  // RIGHT: last interior octet
        }
        RES_MARK(1);
    };
    // refresh the halo of colour plane 1 from the eight neighbours' strips of generation gen
    auto fetch = [&](int gen) {
        RES_MARK(0);
        const int tiles_x = p.tiles_x, tiles_y = R->tiles_y, ntiles = tiles_x * tiles_y;
        const uint64_t tag = strip_tag(gen);
        const int txl = tx == 0 ? tiles_x - 1 : tx - 1, txr = tx == tiles_x - 1 ? 0 : tx + 1;
        const int w_l = txl == tiles_x - 1 ? p.nchunks + p.q_shift - (txl * WO + p.q_shift) : WO;  // lattice octets of the tile column to the left
        const int tyu = ty == 0 ? tiles_y - 1 : ty - 1, tyd = ty == tiles_y - 1 ? 0 : ty + 1;
        const bool has_u = R->wrap_y || ty > 0, has_d = R->wrap_y || ty < tiles_y - 1;
        const bool has_l = R->wrap_x || tx > 0, has_r = R->wrap_x || tx < tiles_x - 1;
        const uint64_t* xg = R->xbuf + (size_t)(gen & 1) * ntiles * xstride;
        const uint64_t* X_u = xg + (size_t)(tyu * tiles_x + tx) * xstride;
        const uint64_t* X_d = xg + (size_t)(tyd * tiles_x + tx) * xstride;
        const uint64_t* X_l = xg + (size_t)(ty * tiles_x + txl) * xstride;
        const uint64_t* X_r = xg + (size_t)(ty * tiles_x + txr) * xstride;
        const uint64_t* X_ul = xg + (size_t)(tyu * tiles_x + txl) * xstride;
        const uint64_t* X_ur = xg + (size_t)(tyu * tiles_x + txr) * xstride;
        const uint64_t* X_dl = xg + (size_t)(tyd * tiles_x + txl) * xstride;
        const uint64_t* X_dr = xg + (size_t)(tyd * tiles_x + txr) * xstride;
        // halo rows: top [0, 2k) from the BOTTOM strips above, bottom [2k + H, TR) from the TOP strips below; halo octets of the
        // interior rows: octet 0 from the left neighbour's RIGHT strip, octet NO-1 from the right one's LEFT.  Every load of
        // a thread is issued before the first is looked at, and unconditionally: a neighbour index always names a real
        // tile, a missing neighbour's value is neither checked nor stored.
        constexpr int FI = (2 * 8 * NO + THREADS - 1) / THREADS;   // k <= 8
        // tallest (stretched slab) tile whose planes fit the CU's LDS (an upper bound: tile_lds_bytes also counts the pair table,
        // the guard octet, the spare row and the tie path's thresholds)
        constexpr int TH_MAX = 160 * 1024 / (int)sizeof(E) / (2 * NO) - 32;
        constexpr int SI = (TH_MAX + THREADS - 1) / THREADS;
        const uint64_t* au[FI];
        const uint64_t* ad[FI];
        uint64_t vu[FI], vd[FI], vl[SI], vr[SI];
        bool nu[FI], nd[FI], nl[SI], nr[SI];  // this thread needs the element
#pragma unroll
        for (int it = 0; it < FI; ++it) {
            const int i = tid + it * THREADS, ic = i < 2 * k * NO ? i : 0;
            const int r = ic / NO, o = ic - r * NO;
            const int e = r * WO;
            const int oc = o <= wi + 1 ? o : 1;  // (octets beyond the right halo: nothing is fetched for them)
            au[it] = oc == 0 ? X_ul + n_tb + e + w_l - 1 : (oc == wi + 1 ? X_ur + n_tb + e : X_u + n_tb + e + oc - 1);
            ad[it] = oc == 0 ? X_dl + e + w_l - 1 : (oc == wi + 1 ? X_dr + e : X_d + e + oc - 1);
            const bool col_ok = o == 0 ? has_l : (o == wi + 1 ? has_r : o <= wi);
            nu[it] = i < 2 * k * NO && has_u && col_ok;
            nd[it] = i < 2 * k * NO && has_d && col_ok;
            vu[it] = xld(au[it]);
            vd[it] = xld(ad[it]);
        }
#pragma unroll
        for (int it = 0; it < SI; ++it) {
            const int i = tid + it * THREADS, ic = i < n_lr ? i : 0;
            nl[it] = i < n_lr && has_l;
            nr[it] = i < n_lr && has_r;
            vl[it] = xld(X_l + 2 * n_tb + n_lr + ic);
            vr[it] = xld(X_r + 2 * n_tb + ic);
        }
        // elements that are not of this generation yet: ask again (a neighbour that finished later; rare and short)
        for (int spins = 0;; ++spins) {
            bool fresh = true;
#pragma unroll
            for (int it = 0; it < FI; ++it) {
                if (nu[it] && (vu[it] & TAG_MASK) != tag) { vu[it] = xld(au[it]); fresh = false; }
                if (nd[it] && (vd[it] & TAG_MASK) != tag) { vd[it] = xld(ad[it]); fresh = false; }
            }
#pragma unroll
            for (int it = 0; it < SI; ++it) {
                const int i = tid + it * THREADS, ic = i < n_lr ? i : 0;
                if (nl[it] && (vl[it] & TAG_MASK) != tag) { vl[it] = xld(X_l + 2 * n_tb + n_lr + ic); fresh = false; }
                if (nr[it] && (vr[it] & TAG_MASK) != tag) { vr[it] = xld(X_r + 2 * n_tb + ic); fresh = false; }
            }
            if (fresh) break;
            // the error flag lives in host memory (a PCIe round trip): look at it rarely
            if (spins > (1 << 22) || ((spins & 0xFFF) == 0xFFF && __hip_atomic_load(R->err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM))) {
                __hip_atomic_store(R->err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);  // ~seconds: grid not co-resident
                s_fail = 1;
                break;
            }
        }
        RES_MARK(2);
#pragma unroll
        for (int it = 0; it < FI; ++it) {
            const int i = tid + it * THREADS;
            if (i < 2 * k * NO) {
                const int r = i / NO, o = i - r * NO;
                if (nu[it]) P.at(1, r, o) = (E)(vu[it] & FLAG_MASK);
                if (nd[it]) P.at(1, 2 * k + H + r, o) = (E)(vd[it] & FLAG_MASK);
            }
        }
#pragma unroll
        for (int it = 0; it < SI; ++it) {
            const int i = tid + it * THREADS;
            if (i < n_lr) {
                if (nl[it]) P.at(1, 2 * k + i, 0) = (E)(vl[it] & FLAG_MASK);
                if (nr[it]) P.at(1, 2 * k + i, wi + 1) = (E)(vr[it] & FLAG_MASK);
            }
        }
        RES_MARK(3);
    };

    // The form of the pair loop is decided once per tile: plain / EDGE / SEAM / OPEN and the column parity par0 of the colour
    // updated in a half-sweep's first row.  Half-sweep hsi starts at tile row 1 + hsi and updates colour hsi & 1; the two always
    // add up to an odd number, so par0 does not change during a launch.
    const int par0 = (int)((p.row0 + Rb + 1) & 1);
    const int form = 2 * (OPEN ? 0 : (seam ? 1 : (edge ? 2 : 3))) + par0;
    // thread (al, oct): LDS byte address of (row 2 al, its octet, plane 0), the start of its pair loop in half-sweep 0
    const uint32_t a_thr = lds_addr(P.base) + (uint32_t)((4 * al * NO + oct) * (int)sizeof(E));
    auto run_generation = [&](uint32_t sweep_g, int kg) {
#define TSU_FORM(P0, EDGE_, OPEN_, SEAM_) sweep_generation<NO, RL, P0, EDGE_, OPEN_, SEAM_, NIB, QUAD>(c, K, TR, sweep_g, kg, a_thr, al, cq)
        if constexpr (OPEN) {
            if (par0) TSU_FORM(1, false, true, false);
            else TSU_FORM(0, false, true, false);
        } else {
            switch (form) {
                case 2: TSU_FORM(0, true, false, true); break;
                case 3: TSU_FORM(1, true, false, true); break;
                case 4: TSU_FORM(0, true, false, false); break;
                case 5: TSU_FORM(1, true, false, false); break;
                case 6: TSU_FORM(0, false, false, false); break;
                default: TSU_FORM(1, false, false, false); break;
            }
        }
#undef TSU_FORM
    };
    for (int gen = 0; gen < n_gen; ++gen) {
    const int kg = (RESIDENT && gen == n_gen - 1) ? R->k_last : k;  // sweeps of this generation (the tile keeps TR = H + 4k)
    const uint32_t sweep_g = sweep0 + (uint32_t)(gen * k);
    // a thread stays on its own octet column and walks every RL-th row pair of each half-sweep's range
    run_generation(sweep_g, kg);
    __syncthreads();
    if (RESIDENT && gen + 1 < n_gen) {
        publish(gen);
        fetch(gen);
        __syncthreads();
        if (s_fail) return;  // nothing is stored: the source buffer stays valid
    }
    RES_MARK(0);
    }  // generations
    if (timing)
        for (int q = 0; q < 4; ++q) R->dbg[4 * blockIdx.x + q] = tl[q];
#undef RES_MARK
    // interior octets are tile columns 1 .. NO-2: the same thread -> column mapping, halo columns idle
    if (al < RLMAX && oct >= 1 && oct <= WO && q0 + oct - 1 < p.nchunks + p.q_shift) {
        int8_t* col = dst + 16 * (long long)cqi;  // (= q0 + oct - 1, wrapped when the tiling starts at octet q_shift)
        int gpar = (int)((p.row0 + r0 + al) & 1);
#pragma unroll 2
        for (int hr = al; hr < H; hr += RLMAX) {
            const int rl = r0 + hr;
            if (rl < p.r_end) {
                uint64_t ev = P.at(gpar, 2 * k + hr, oct), od = P.at(gpar ^ 1, 2 * k + hr, oct);
                if (NIB) {  // nibble octet -> byte-per-site flags
                    ev = (ev & 0x01010101ull) | (((ev >> 4) & 0x01010101ull) << 32);
                    od = (od & 0x01010101ull) | (((od >> 4) & 0x01010101ull) << 32);
                }
                if (QUAD) {  // the flag as 0 / 1, which the look-up below selects by
                    ev >>= QUAD_SHIFT;
                    od >>= QUAD_SHIFT;
                }
                // up flag -> spin byte: 1 -> 0x01, 0 -> 0xFF
                const uint32_t e0 = perm(0u, 0x000001FFu, (uint32_t)ev), e1 = perm(0u, 0x000001FFu, (uint32_t)(ev >> 32));
                const uint32_t o0 = perm(0u, 0x000001FFu, (uint32_t)od), o1 = perm(0u, 0x000001FFu, (uint32_t)(od >> 32));
                uint4 v = make_uint4(perm(o0, e0, 0x05010400u), perm(o0, e0, 0x07030602u), perm(o1, e1, 0x05010400u),
                                     perm(o1, e1, 0x07030602u));
                if (nv < 16) {  // ragged last chunk: the pad bytes of the row stay 0
                    auto bytes = [](int n) { return n >= 4 ? 0xFFFFFFFFu : (n <= 0 ? 0u : (1u << (8 * n)) - 1u); };
                    v.x &= bytes(nv);
                    v.y &= bytes(nv - 4);
                    v.z &= bytes(nv - 8);
                    v.w &= bytes(nv - 12);
                }
                *reinterpret_cast<uint4*>(col + (long long)rl * p.pitch) = v;
            }
            if (RLMAX & 1) gpar ^= 1;
        }
    }
}

template <int H, int WO, int THREADS, int MINW = 1, bool OPEN = false, bool NIB = false, bool QUAD = false>
__global__ __launch_bounds__(THREADS, MINW) void k1_tiled2(TiledParams p) {
    extern __shared__ uint64_t lds[];
    const PhiloxKeys K = make_keys(p.k0, p.k1);
    tile_body<H, WO, THREADS, OPEN, false, NIB, QUAD>(p, p.src, p.dst, p.k, p.sweep0, blockIdx.x % p.tiles_x,
                                    p.ty_first + (blockIdx.x / p.tiles_x) * p.ty_stride, lds, K);
}

// ------------------------------------------------------------------ tile-resident multi-generation kernel
struct ResidentLaunch {
    TiledParams t;
    ResidentParams r;
};

template <int H, int WO, int THREADS, int MINW = 1, bool OPEN = false, bool NIB = false, bool QUAD = false>
__global__ __launch_bounds__(THREADS, MINW) void k1_resident(ResidentLaunch P) {
    extern __shared__ uint64_t lds[];
    const PhiloxKeys K = make_keys(P.t.k0, P.t.k1);
    tile_body<H, WO, THREADS, OPEN, true, NIB, QUAD>(P.t, P.t.src, P.t.dst, P.t.k, P.t.sweep0, blockIdx.x % P.t.tiles_x, blockIdx.x / P.t.tiles_x,
                                          lds, K, &P.r);
}

// ------------------------------------------------------------------ host side
namespace {
constexpr int KMAX = 8;  // one halo octet (16 columns) covers 2k <= 16 half-sweeps

struct TileVariant {
    int H, WO, threads;
    void (*kernel)(TiledParams);
    void (*resident)(ResidentLaunch);  // tile-resident multi-generation form (nullptr: not built for this shape)
    void (*open)(TiledParams);       // open-boundary form (nullptr: not built for this shape)
    void (*resident_open)(ResidentLaunch);
    int nib;                         // colour planes at 4 bits per site (periodic lattices, width a multiple of 16)
    int per_cu;                      // workgroups of this shape one CU is meant to hold (tiles per round; LDS share of a stretched tile)
    void (*kernel_q)(TiledParams);   // periodic byte planes with the quad threshold table (nullptr: nibble planes keep the pair table)
    void (*resident_q)(ResidentLaunch);
};

// LDS of one workgroup: pair table, guard octet, two colour planes of TR x NO octets (+ one spare row), 25 thresholds
size_t tile_lds_bytes(const TileVariant& tv, int TR, bool quad = false) {
    const size_t es = tv.nib ? 4 : 8, NO = (size_t)tv.WO + 2;
    return 8 * (quad ? TBL4_OCTETS : TBL2_OCTETS) + 8 + (((size_t)2 * TR * NO + NO + 1) * es + 7) / 8 * 8 + 8 + 25 * sizeof(uint64_t);
}
// the tile shapes the chooser (plan_call) can reach.  Round 1's table had 32 entries, 24 of them reachable only through
// the TSU_TILE_VARIANT development switch; numbers quoted in profiles/r01_* map as 6 -> 0, 8 -> 1, 9 -> 2, 22 -> 3, 23 -> 4,
// 25 -> 5, 26 -> 6, 27 -> 7
enum { V_64x512_T512 = 0, V_128x512_T512, V_128x512_T1024, V_256x512_T1024, V_128x256_T1024, V_64x512_T1024, V_64x256_T1024, V_32x256_T1024,
       V_N512x512_T1024, V_N256x512_T512 };
const TileVariant kVariants[] = {
    {64, 32, 512, k1_tiled2<64, 32, 512>, k1_resident<64, 32, 512>, k1_tiled2<64, 32, 512, 1, true>, nullptr, 0, 2,
     k1_tiled2<64, 32, 512, 1, false, false, true>, k1_resident<64, 32, 512, 1, false, false, true>},
    {128, 32, 512, k1_tiled2<128, 32, 512>, k1_resident<128, 32, 512>, k1_tiled2<128, 32, 512, 1, true>, nullptr, 0, 2,
     k1_tiled2<128, 32, 512, 1, false, false, true>, k1_resident<128, 32, 512, 1, false, false, true>},
    {128, 32, 1024, k1_tiled2<128, 32, 1024>, k1_resident<128, 32, 1024>, k1_tiled2<128, 32, 1024, 1, true>, k1_resident<128, 32, 1024, 1, true>, 0, 1,
     k1_tiled2<128, 32, 1024, 1, false, false, true>, k1_resident<128, 32, 1024, 1, false, false, true>},
    {256, 32, 1024, k1_tiled2<256, 32, 1024, 4>, k1_resident<256, 32, 1024, 4>, k1_tiled2<256, 32, 1024, 4, true>, k1_resident<256, 32, 1024, 4, true>, 0, 1,
     k1_tiled2<256, 32, 1024, 4, false, false, true>, k1_resident<256, 32, 1024, 4, false, false, true>},  // one 148 KB workgroup per CU
    {128, 16, 1024, k1_tiled2<128, 16, 1024>, k1_resident<128, 16, 1024>, k1_tiled2<128, 16, 1024, 1, true>, k1_resident<128, 16, 1024, 1, true>, 0, 1,
     k1_tiled2<128, 16, 1024, 1, false, false, true>, k1_resident<128, 16, 1024, 1, false, false, true>},  // narrower tiles for mid-size lattices
    {64, 32, 1024, k1_tiled2<64, 32, 1024>, k1_resident<64, 32, 1024>, k1_tiled2<64, 32, 1024, 1, true>, k1_resident<64, 32, 1024, 1, true>, 0, 1,
     k1_tiled2<64, 32, 1024, 1, false, false, true>, k1_resident<64, 32, 1024, 1, false, false, true>},
    {64, 16, 1024, k1_tiled2<64, 16, 1024>, k1_resident<64, 16, 1024>, k1_tiled2<64, 16, 1024, 1, true>, k1_resident<64, 16, 1024, 1, true>, 0, 1,
     k1_tiled2<64, 16, 1024, 1, false, false, true>, k1_resident<64, 16, 1024, 1, false, false, true>},
    {32, 16, 1024, k1_tiled2<32, 16, 1024>, k1_resident<32, 16, 1024>, k1_tiled2<32, 16, 1024, 1, true>, k1_resident<32, 16, 1024, 1, true>, 0, 1,
     k1_tiled2<32, 16, 1024, 1, false, false, true>, k1_resident<32, 16, 1024, 1, false, false, true>},
    // nibble planes: 512 x 512 sites per CU (148 KB) -- 8192^2 tile-resident; 256 x 512, two workgroups per CU, for what is larger still
    {512, 32, 1024, k1_tiled2<512, 32, 1024, 4, false, true>, k1_resident<512, 32, 1024, 4, false, true>, k1_tiled2<512, 32, 1024, 4, true, true>,
     k1_resident<512, 32, 1024, 4, true, true>, 1, 1, nullptr, nullptr},
    {256, 32, 512, k1_tiled2<256, 32, 512, 4, false, true>, nullptr, k1_tiled2<256, 32, 512, 4, true, true>, nullptr, 1, 2, nullptr, nullptr},
};
constexpr int kNumVariants = sizeof(kVariants) / sizeof(kVariants[0]);

// A periodic lattice whose width is not a multiple of 16 has a ragged last octet (v < 8 sites per colour).  As a halo
// octet it would give a tile 2v columns of history instead of 16, so the tiling starts at octet `shift` such that the
// ragged octet is never the left halo of a tile (tile start = 0 mod nch) nor the right halo of any but the last tile.
// 0: not needed; -1: no such start (the generic kernel takes the lattice).
int ragged_shift(const tsu_ising2d* L, int WO) {
    if (!L->periodic || L->cols % 16 == 0) return 0;
    const int nch = (L->cols + 15) / 16, tiles_x = (nch + WO - 1) / WO;
    for (int shift = 1; shift < WO && shift < nch - 1; ++shift) {
        bool ok = true;
        for (int t = 0; t < tiles_x && ok; ++t) {
            const int s = t * WO + shift;
            if (s % nch == 0) ok = false;
            if (t < tiles_x - 1 && (s + WO) % nch == nch - 1) ok = false;
        }
        if (ok) return shift;
    }
    return -1;
}

// LDS of one workgroup of this shape when per_cu of them share a CU
size_t lds_share(const TileVariant& tv) { return (size_t)(160 / tv.per_cu) * 1024; }

// The quad threshold table (pair_thresholds) is 4.9 KB larger than the pair table.  Tile shapes, heights and cuts are planned with
// the pair table's size, as before; a launch whose tile of TR rows leaves room for the larger table within the variant's LDS share
// takes the quad kernels, every other launch the pair-table ones: no lattice gets another plan.  (The tallest byte tile planned,
// 256 + 32 rows of variant 3, uses 158.4 of 160 KB with it.)
bool quad_fits(const tsu_ising2d* L, const TileVariant& tv, int TR) {
    return L->periodic && tv.kernel_q && tile_lds_bytes(tv, TR, true) <= lds_share(tv);
}

// CUs of the lattice's device (256 when unknown)
int chip_cus(const tsu_ising2d* L) { return L->ctx->cus > 0 ? L->ctx->cus : 256; }

// an integer switch from the environment (unset: dflt)
int lattice_env(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

// Generation time (us) of k = 8 sweeps on tiles of h rows, fitted to measurements (4096^2, 2048^2, 1024^2, 4096 x 8192, open
// 1000^2; profiles/r01_k1_experiments.txt): a half-sweep costs 0.25 us + 0.225 us per wave-iteration of the busiest SIMD (6 %
// more on nibble planes); between generations `between` us: the strip exchange costs 4.3 us when the tiles stay resident in LDS,
// the tile store + launch gap + stage about 12 us when they do not.  (The fit is older than the counted-down EDGE form of
// edge_rows, which took about 0.1 us per sweep off 4096^2 and 0.2 us off 8192^2, and older than the row wrap in the Philox head,
// which took another 0.05 us and 0.4 us off them (profiles/k1_row_mask_ab.txt).  It has not been re-fitted: the chooser compares
// shapes for one lattice, and both changes shorten the generations of every shape on that lattice's height alike.)
double gen_time_us(const TileVariant& c, int h, double between) {
    const int pairs = (h + 4 * 8 - 2) / 2, waves = (pairs * (c.WO + 2) + 63) / 64;
    return 16.0 * (0.25 + (c.nib ? 1.06 : 1.0) * 0.225 * ((waves + 3) / 4)) + between;
}

// thresholds of a TiledParams / PlanesItem: the full table (tie path) and its top 16 bits, min(thr >> 16, 65535) ^ 0x8000, as byte
// tables for degree 4 (tbl*) and, for open lattices, degree 3 (t3*, entries 0..3) and degree 2 (entries 4..6)
template <typename P>
void pack_thresholds(P& p, const uint64_t table[25]) {
    for (int c = 0; c < 25; ++c) p.thr[c] = table[c];
    auto top16 = [](uint64_t thr) {
        uint32_t thi = (uint32_t)(thr >> 16);
        if (thi > 65535u) thi = 65535u;
        return thi ^ 0x8000u;
    };
    uint32_t t16[5], t3[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int c = 0; c < 5; ++c) t16[c] = top16(table[4 * 5 + c]);
    for (int c = 0; c < 4; ++c) t3[c] = top16(table[3 * 5 + c]);      // degree 3: an edge
    for (int c = 0; c < 3; ++c) t3[4 + c] = top16(table[2 * 5 + c]);  // degree 2: a corner
    p.t3L0 = (t3[0] & 0xFF) | ((t3[1] & 0xFF) << 8) | ((t3[2] & 0xFF) << 16) | ((t3[3] & 0xFF) << 24);
    p.t3L1 = (t3[4] & 0xFF) | ((t3[5] & 0xFF) << 8) | ((t3[6] & 0xFF) << 16);
    p.t3H0 = (t3[0] >> 8) | ((t3[1] >> 8) << 8) | ((t3[2] >> 8) << 16) | ((t3[3] >> 8) << 24);
    p.t3H1 = (t3[4] >> 8) | ((t3[5] >> 8) << 8) | ((t3[6] >> 8) << 16);
    p.tblL0 = (t16[0] & 0xFF) | ((t16[1] & 0xFF) << 8) | ((t16[2] & 0xFF) << 16) | ((t16[3] & 0xFF) << 24);
    p.tblL1 = (t16[4] & 0xFF);
    p.tblH0 = (t16[0] >> 8) | ((t16[1] >> 8) << 8) | ((t16[2] >> 8) << 16) | ((t16[3] >> 8) << 24);
    p.tblH1 = (t16[4] >> 8);
}

// Tile-resident runs of whole lattices of any shape (flexible cut; periodic ones need even height and width): the rows are
// cut into tiles_y tile rows of (nearly) equal even heights and the last tile column may hold fewer octets than the others, so
// the lattice need not divide into whole tiles.  As many tile rows as the chip has room for (every tile needs its own
// workgroup; more tiles = shorter tiles = a shorter generation), the tile shape by the generation-time model.
// Returns tiles_y (0: no such cut) for variant v, or searches the variants when v < 0 and returns the best through *v_out.
int flex_cut(const tsu_ising2d* L, int v, int* v_out, int* hmax_out, double* t_out) {
    if (L->ghost != 0 || L->total_rows != L->rows) return 0;
    if (L->periodic && ((L->cols & 1) || (L->rows & 1))) return 0;  // (odd periodic lattices are not bipartite: generic kernel)
    const int FLEX_HMIN = 16;  // shortest tile row of a cut (the strips are 2k = 16 rows deep)
    static const int max_tiles = lattice_env("TSU_K1_FLEX_MAX_TILES", 0);  // test switch: pretend the chip has room for this many tiles only
    int cus = chip_cus(L);
    if (max_tiles > 0 && max_tiles < cus) cus = max_tiles;
    const int nch = (L->cols + 15) / 16;
    static const int cand[] = {V_256x512_T1024, V_128x256_T1024, V_N512x512_T1024};
    double best = 1e300;
    int best_ty = 0;
    for (int ci = 0; ci < (int)(sizeof(cand) / sizeof(cand[0])); ++ci) {
        if (v >= 0 && cand[ci] != v) continue;
        const TileVariant& c = kVariants[cand[ci]];
        if (!(L->periodic ? c.resident : c.resident_open) || 2 * nch < c.WO || ragged_shift(L, c.WO) < 0) continue;
        // (an open lattice may have an odd number of rows: the cut is made over rows + 1, the last tile row holds one row less)
        const int tiles_x = (nch + c.WO - 1) / c.WO, half = (L->rows + 1) / 2;
        int tiles_y = cus / tiles_x;
        if (tiles_y > half / (FLEX_HMIN / 2)) tiles_y = half / (FLEX_HMIN / 2);  // a small lattice: not every CU gets a tile
        if (tiles_y < 1) continue;
        const int hmax = 2 * ((half + tiles_y - 1) / tiles_y), hmin = 2 * (half / tiles_y);
        if (hmin < FLEX_HMIN || L->total_rows < hmax + 4 * KMAX || tile_lds_bytes(c, hmax + 4 * KMAX) > 160 * 1024) continue;
        const double t_gen = gen_time_us(c, hmax, 4.3);
        if (t_gen < best) {
            best = t_gen;
            best_ty = tiles_y;
            *v_out = cand[ci];
            *hmax_out = hmax;
        }
    }
    *t_out = best;
    return best_ty;
}

// Everything a tiled call of n_sweeps sweeps over `part` needs.  The first half is the lattice's: its tile shape and flexible cut
// (tsu_ising2d_tiled_tiles / _supported / _part_supported read those); the second half the call's.
struct CallPlan {
    int v;                // index into kVariants; -1: no tile shape fits (the generic kernel takes the lattice)
    int flex_ty, flex_h;  // the lattice's flexible cut: tile rows and the tallest of them (0: none; whole lattices only)
    int kmax;             // sweeps per launch, or per generation of a tile-resident run
    bool resident;        // tile-resident generations, if every tile finds its workgroup on the chip (checked at launch)
    int tile_h, tiles_y;  // the resident run's tiles: the flexible cut, whole tiles, or a slab's tiles stretched over ...
    int res_ext;          // ... this many ghost rows on each side
};

CallPlan plan_call(const tsu_ising2d* L, int n_sweeps, int part) {
    CallPlan c{};
    static const int env = lattice_env("TSU_TILE_VARIANT", -1);  // test switch: force a tile shape
    const bool forced = env >= 0 && env < kNumVariants;
    const int cus = chip_cus(L), nch = (L->cols + 15) / 16;
    const bool whole_lattice = L->ghost == 0 && L->total_rows == L->rows;
    int v;
    if (forced) {
        v = env;
    } else {
        // measured on MI355X (profiles/r01_k1_experiments.txt): 128-row tiles with two 512-thread workgroups per CU
        // when the lattice gives every CU several tiles; a lattice with at most one such tile per CU needs all 16
        // waves of the CU in one workgroup; one with ABOUT TWO per CU (2048 x 16384, 4096 x 8192: everything starts
        // and ends together, nothing hides the stage/store phases) does better with 256-row tiles, one per CU
        const long long tx = (nch + 31) / 32;
        const long long n128 = ((L->rows + 127) / 128) * tx, n256 = ((L->rows + 255) / 256) * tx;
        if (n128 <= cus) v = V_128x512_T1024;
        else if (n128 <= 2 * cus && n256 <= cus && 10 * n256 >= 7 * cus) v = V_256x512_T1024;
        else v = V_128x512_T512;
        if (L->rows < 256) v = V_64x512_T512;
        // Nibble planes (whole lattices; any width: an open lattice's ragged last octet is masked like every site beyond the
        // edge, a periodic one's takes the SEAM form): a lattice of exactly one 512 x 512 tile per CU (8192^2 on 256 CUs) stays
        // resident in LDS; larger lattices take 256 x 512 tiles, two workgroups per CU, 8 sweeps per launch (half the halo rows
        // of the 128-row byte tiles and fewer stage/store passes)
        if (whole_lattice && n128 > 2 * cus) {
            const long long n512 = (long long)(L->rows / 512) * (nch / 32);
            if (L->rows % 512 == 0 && nch % 32 == 0 && n512 <= cus && 2 * n512 > cus) v = V_N512x512_T1024;
            else if (L->rows >= 512) v = V_N256x512_T512;
        }
        // Lattices that give every CU at most one tile: the tile shape that finishes a generation of 8 sweeps soonest
        static const int cand[] = {V_256x512_T1024, V_128x512_T1024, V_128x256_T1024, V_64x512_T1024, V_64x256_T1024, V_32x256_T1024};
        double best = 1e30;
        for (int ci = 0; whole_lattice && ci < (int)(sizeof(cand) / sizeof(cand[0])); ++ci) {
            const TileVariant& t = kVariants[cand[ci]];
            if (!(L->periodic ? t.kernel : t.open)) continue;
            if (2 * nch < t.WO || L->total_rows < t.H + 4 * KMAX || ragged_shift(L, t.WO) < 0) continue;
            const long long nt = (long long)((L->rows + t.H - 1) / t.H) * ((nch + t.WO - 1) / t.WO);
            if (nt > cus) continue;
            const bool resident = (L->periodic ? t.resident : t.resident_open) && L->rows % t.H == 0 && nch % t.WO == 0;
            const double t_gen = gen_time_us(t, t.H, resident ? 4.3 : 12.0);
            if (t_gen < best) {
                best = t_gen;
                v = cand[ci];
            }
        }
    }
    // a whole periodic lattice that the pick above cannot keep resident in LDS (it does not divide into that shape's tiles, or
    // has more of them than the chip has room for) takes the flexible cut if one exists
    // ... and so does one that the pick above keeps resident in fewer, taller tiles than the chip has room for (6144^2 in 512-row
    // nibble tiles: 144 tiles on 256 CUs) when the model gives the flexible cut a generation that is at least 3 % shorter.
    {
        const TileVariant& t = kVariants[v];
        const long long nt = (long long)((L->rows + t.H - 1) / t.H) * ((nch + t.WO - 1) / t.WO);
        const bool divides = L->rows % t.H == 0 && nch % t.WO == 0;
        const bool standard_resident = (L->periodic ? t.resident : t.resident_open) && divides && nt <= (long long)t.per_cu * cus;
        int fv = -1, fh = 0;
        double t_flex = 0;
        const int fty = forced ? (divides ? 0 : flex_cut(L, v, &fv, &fh, &t_flex)) : flex_cut(L, -1, &fv, &fh, &t_flex);
        bool take = fty > 0 && !standard_resident;
        // a batch of lattices (a temperature scan on side streams) wants many lattices in flight, not the shortest generation of
        // one: lattices that leave half the chip to the others keep the tuned, compact shapes (32 temperatures at 1024^2: 120 ms;
        // with every lattice cut into 256 tiles 182 ms)
        const bool compact = L->ctx->in_batch && 2 * nt <= cus;
        if (compact) take = false;
        if (fty > 0 && standard_resident && !forced && t.per_cu == 1 && !compact) take = t_flex < 0.97 * gen_time_us(t, t.H, 4.3);
        if (take) {
            v = fv;
            c.flex_ty = fty;
            c.flex_h = fh;
        }
    }
    // a variant must fit the lattice (a tile is a window on the lattice's periodic extension: its octet and row indices
    // wrap at most twice / once) and, for an open lattice, have the OPEN form built; -1 = none does (generic kernel)
    auto fits = [&](int vv) {
        return 2 * nch >= kVariants[vv].WO && L->total_rows >= kVariants[vv].H + 4 * KMAX && (L->periodic || kVariants[vv].open) &&
               ragged_shift(L, kVariants[vv].WO) >= 0;
    };
    if (!fits(v)) {
        static const int fallback[] = {V_64x512_T512, V_64x256_T1024, V_32x256_T1024};
        v = -1;
        c.flex_ty = c.flex_h = 0;
        for (int f : fallback)
            if (fits(f)) {
                v = f;
                break;
            }
    }
    c.v = v;
    if (v < 0) return c;

    const TileVariant& tv = kVariants[v];
    // sweeps per launch: more sweeps amortise the tile load/store and the launch gap, fewer carry less halo work
    // (one workgroup per CU, or a small lattice: 8; large lattices with two workgroups per CU that overlap each other's
    // stage/store phases: 5)
    c.kmax = L->sweeps_per_launch > 0 ? L->sweeps_per_launch : ((tv.nib || tv.threads >= 1024 || (long long)L->rows * L->cols <= 4096ll * 4096ll) ? 8 : 5);
    if (c.kmax > KMAX) c.kmax = KMAX;
    c.tile_h = tv.H;
    c.tiles_y = (L->rows + tv.H - 1) / tv.H;
    static const int use_resident = lattice_env("TSU_K1_RESIDENT", 1);
    c.resident = use_resident && (L->periodic ? tv.resident : tv.resident_open) && part == TSU_PART_ALL && n_sweeps > c.kmax;
    const bool whole = L->wrap_rows || (!L->periodic && whole_lattice);
    if (!c.resident) return c;
    if (whole && c.flex_ty > 0) {  // the flexible cut: balanced tile rows, a partial last tile column
        c.tile_h = c.flex_h;
        c.tiles_y = c.flex_ty;
    } else if (whole) {  // whole tiles of tv.H x tv.WO
        c.resident = nch % tv.WO == 0 && L->rows % tv.H == 0;
    } else {
        // periodic slab: its tiles stretched over the ghost rows that the call's later generations need (uniform even height
        // th, th * tiles_y = rows + 2 ext, 2 (n_sweeps - k) <= ext <= ghost)
        const int need = L->rows + 4 * (n_sweeps - c.kmax);
        int th = (need + c.tiles_y - 1) / c.tiles_y;
        th += th & 1;
        if (th < tv.H) th = tv.H;
        const int extra = th * c.tiles_y - L->rows;
        c.tile_h = th;
        c.res_ext = extra / 2;
        c.resident = nch % tv.WO == 0 && extra % 2 == 0 && c.res_ext <= L->ghost && tile_lds_bytes(tv, th + 4 * c.kmax) <= lds_share(tv);
    }
    return c;
}

// Tile rows of one launch of k sweeps in the launch-per-generation form, `left` sweeps of the call still to do: sets p.tile_h,
// p.r_begin and p.r_end and returns the number of tile rows.
int launch_tiles(const tsu_ising2d* L, const TileVariant& tv, int k, int left, int part, bool slab, TiledParams& p) {
    p.tile_h = tv.H;
    p.r_begin = 0;
    p.r_end = L->rows;
    if (part != TSU_PART_ALL) return (L->rows + tv.H - 1) / tv.H;
    if (!slab) {
        // A whole lattice: any even height the variant's LDS share holds gives the same results, so it is chosen for the schedule.
        // The chip runs `slots` tiles at a time and a tile costs about (th + 2k + 12) row times (its trapezoid of halo rows, its
        // stage and store), so a lattice costs ceil(tiles / slots) rounds of that: 10000^2 in 256-row nibble tiles is 800 tiles on
        // 512 slots -- two rounds, the second 56 % full; in 198-row tiles it is 1020 tiles, two full rounds of shorter tiles
        // (-21 %).  Lattices with fewer tiles than slots get shorter tiles so that every slot has one.
        const long long slots = (long long)tv.per_cu * chip_cus(L);
        double best = 1e300;
        for (int th = 32; th <= 1024; th += 2) {
            if (th + 4 * KMAX > L->total_rows || tile_lds_bytes(tv, th + 4 * k) > lds_share(tv)) continue;
            const long long nt = (long long)((L->rows + th - 1) / th) * p.tiles_x, rounds = (nt + slots - 1) / slots;
            const double cost = (double)rounds * (th + 2 * k + 12);
            if (cost < best * (1.0 - 1e-9) || (cost <= best * (1.0 + 1e-9) && th > p.tile_h)) {
                best = cost;
                p.tile_h = th;
            }
        }
        return (L->rows + p.tile_h - 1) / p.tile_h;
    }
    // A slab computes the ghost rows its remaining sweeps of this refresh period need, 2 per sweep on each side.  It keeps the
    // number of tile rows (an extra, nearly empty tile row can cost a whole extra round of tiles): the tiles stretch instead, if
    // the taller tile still fits the LDS share this variant runs with
    const int ext = 2 * (left - k);
    p.r_begin = -ext;
    p.r_end = L->rows + ext;
    const int base_ty = (L->rows + tv.H - 1) / tv.H;
    int th = (p.r_end - p.r_begin + base_ty - 1) / base_ty;
    th += th & 1;
    if (th >= tv.H && tile_lds_bytes(tv, th + 4 * k) <= lds_share(tv)) p.tile_h = th;
    return (p.r_end - p.r_begin + p.tile_h - 1) / p.tile_h;
}

// TSU_K1_VERBOSE >= 2: the in-kernel timeline of a tile-resident launch, [ntiles][4] clock counts (10 ns) per tile
void print_resident_timeline(const long long* d_dbg, int ntiles, int tiles_x, int tiles_y, int n_gen, int verbose) {
    std::vector<long long> h((size_t)4 * ntiles);
    (void)hipMemcpy(h.data(), d_dbg, h.size() * sizeof(long long), hipMemcpyDeviceToHost);
    static const char* const what[4] = {"sweeps", "publish", "wait", "fetch"};
    fprintf(stderr, "[tsu]   us per generation over %d tiles (mean / min / max):", ntiles);
    for (int q = 0; q < 4; ++q) {
        double sum = 0, lo = 1e30, hi = 0;
        for (int t = 0; t < ntiles; ++t) {
            const double v = h[(size_t)4 * t + q] / 100.0 / n_gen;
            sum += v;
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
        }
        fprintf(stderr, " %s %.1f / %.1f / %.1f%s", what[q], sum / ntiles, lo, hi, q < 3 ? "," : "\n");
    }
    if (verbose < 3) return;
    for (int x = 0; x < 8; ++x) {  // by XCD (workgroup index mod 8): does one die run behind the others?
        double sw = 0, wt = 0;
        int cnt = 0;
        for (int t = x; t < ntiles; t += 8, ++cnt) {
            sw += h[(size_t)4 * t] / 100.0 / n_gen;
            wt += h[(size_t)4 * t + 2] / 100.0 / n_gen;
        }
        if (cnt) fprintf(stderr, "[tsu]   xcd %d: sweeps %.2f wait %.2f\n", x, sw / cnt, wt / cnt);
    }
    if (verbose < 4) return;
    for (int y = 0; y < tiles_y; ++y) {  // the whole map: sweeps / wait per tile, one line per tile row
        fprintf(stderr, "[tsu]   row %3d:", y);
        for (int x = 0; x < tiles_x; ++x)
            fprintf(stderr, " %.1f/%.1f", h[(size_t)4 * (y * tiles_x + x)] / 100.0 / n_gen, h[(size_t)4 * (y * tiles_x + x) + 2] / 100.0 / n_gen);
        fprintf(stderr, "\n");
    }
}

// ---- tile-resident generations: every tile has its own workgroup on the chip for the whole call (fit_per_cu: the occupancy check's)
int run_resident(tsu_ising2d* L, const CallPlan& c, TiledParams p, int n_sweeps, uint32_t sweep0, int fit_per_cu, bool quad) {
    tsu_ctx* ctx = L->ctx;
    const TileVariant& tv = kVariants[c.v];
    void (*const res_kern)(ResidentLaunch) = quad ? tv.resident_q : (L->periodic ? tv.resident : tv.resident_open);
    const int kmax = c.kmax, ntiles = p.tiles_x * c.tiles_y;
    const bool whole = L->wrap_rows || (!L->periodic && L->ghost == 0 && L->total_rows == L->rows);
    const size_t lds_bytes = tile_lds_bytes(tv, c.tile_h + 4 * kmax, quad);
    const size_t xstride = (size_t)2 * (2 * kmax * tv.WO) + (size_t)2 * c.tile_h;  // TOP, BOTTOM, LEFT, RIGHT of colour plane 1
    const size_t xneed = (size_t)2 * ntiles * xstride;
    if (L->xbuf_cap < xneed * sizeof(uint64_t)) L->xsig = 0;  // fresh memory: cleared before its first use below
    TSU_HIP_TRY(ctx, ising2d_grow(L->d_xbuf, L->xbuf_cap, xneed * sizeof(uint64_t)));
    // strip layout of this call: the element numbering may only run on while it stays the same
    const uint64_t xsig = ((uint64_t)(c.v + 1) << 48) ^ ((uint64_t)ntiles << 28) ^ ((uint64_t)kmax << 20) ^ ((uint64_t)c.tile_h << 4) ^
                          ((uint64_t)c.flex_ty << 36) ^ (uint64_t)p.open ^ ((uint64_t)quad << 1);  // (quad: other flag and number bits)
    int* d_err = nullptr;
    if (const int rc = tsu_err_flag(ctx, L->h_err, &d_err); rc != TSU_OK) return rc;
    const int verbose = lattice_env("TSU_K1_VERBOSE", 0);
    // one launch per 1024 generations at most (a whole lattice may be asked for millions of sweeps; a slab's call
    // is one refresh period anyway)
    const int chunk_max = whole ? 1024 * kmax : n_sweeps;
    for (int done = 0; done < n_sweeps;) {
        const int chunk = n_sweeps - done < chunk_max ? n_sweeps - done : chunk_max;
        ResidentLaunch P;
        p.k = kmax;
        p.sweep0 = sweep0 + (uint32_t)done;
        p.ty_first = 0;
        p.ty_stride = 1;
        p.src = L->alloc[L->cur] + (size_t)L->ghost * L->pitch;
        p.dst = L->alloc[L->cur ^ 1] + (size_t)L->ghost * L->pitch;
        p.tile_h = c.tile_h;
        p.flex_ty = c.flex_ty;
        p.r_begin = -c.res_ext;
        p.r_end = L->rows + c.res_ext;
        P.t = p;
        P.r.wrap_y = L->wrap_rows ? 1 : 0;
        P.r.wrap_x = L->periodic ? 1 : 0;
        P.r.xbuf = L->d_xbuf;
        const bool renumber = L->xsig != xsig || L->xgen + (uint32_t)((chunk + kmax - 1) / kmax) + 2u >= 16383u;
        if (renumber) {
            L->xrestarts += 1;
            L->xsig = xsig;
            L->xgen = 0;
        }
        P.r.gen0 = L->xgen + 1u;
        L->xgen += (uint32_t)((chunk + kmax - 1) / kmax);
        P.r.err = d_err;
        P.r.n_gen = (chunk + kmax - 1) / kmax;
        P.r.k_last = chunk - (P.r.n_gen - 1) * kmax;
        P.r.tiles_y = c.tiles_y;
        P.r.dbg = nullptr;
        long long* d_dbg = nullptr;
        if (verbose >= 2) {
            TSU_HIP_TRY(ctx, hipMalloc(&d_dbg, (size_t)4 * ntiles * sizeof(long long)));
            P.r.dbg = d_dbg;
        }
        if (verbose) {
            // how the tiles whose windows hold the lattice's wrap row take it (tile_body): in the Philox head or in the EDGE loop
            bool any_wrap = false;
            for (int ty = 0; ty < c.tiles_y && !any_wrap; ++ty) {
                long long rg0;
                any_wrap = tile_holds_wrap(P.t, ty, kmax, rg0);
            }
            fprintf(stderr, "[tsu] k1_resident variant %d: %d tiles (%d per CU fit), %d generations of %d sweeps, %zu KB of strips, thresholds: %s, row wrap: %s\n",
                    c.v, ntiles, fit_per_cu, P.r.n_gen, kmax, xneed * 8 / 1024, quad ? "quad table" : (L->periodic ? "pair table" : "v_perm"),
                    !any_wrap ? "none" : (wrap_by_mask(P.t) ? "mask" : "compare"));
        }
        {
            const int rcx = tsu_grid_exclusive_begin(ctx);
            if (rcx != TSU_OK) return rcx;
        }
        // the numbering restarts (or another strip layout starts): no element may look like one of the new run
        // (after the chaining above: an earlier launch of this lattice on another stream has finished with the buffer)
        if (renumber) TSU_HIP_TRY(ctx, hipMemsetAsync(L->d_xbuf, 0, L->xbuf_cap, ctx->stream));
        // (a slab's launches alternate with the halo exchange's RCCL kernels on this stream: ordinary launch, see tsu_launch_grid_sync)
        TSU_HIP_TRY(ctx, tsu_launch_grid_sync(ctx, (const void*)res_kern, dim3((unsigned)ntiles), dim3((unsigned)tv.threads), &P, lds_bytes, ctx->stream,
                                              !whole));
        L->launches += 1;
        L->cur ^= 1;
        {
            const int rcx = tsu_grid_exclusive_end(ctx);
            if (rcx != TSU_OK) return rcx;
        }
        if (d_dbg) {
            print_resident_timeline(d_dbg, ntiles, p.tiles_x, c.tiles_y, P.r.n_gen, verbose);
            (void)hipFree(d_dbg);
        }
        done += chunk;
    }
    return TSU_OK;
}

// ---- one launch per k <= kmax sweeps, out of place (the host ping-pongs the lattice buffers)
int run_generations(tsu_ising2d* L, const CallPlan& c, TiledParams p, int n_sweeps, uint32_t sweep0, int part) {
    tsu_ctx* ctx = L->ctx;
    const TileVariant& tv = kVariants[c.v];
    const bool slab = !(L->wrap_rows || (!L->periodic && L->ghost == 0 && L->total_rows == L->rows));
    const int verbose = lattice_env("TSU_K1_VERBOSE", 0);
    for (int done = 0; done < n_sweeps;) {
        const int k = n_sweeps - done < c.kmax ? n_sweeps - done : c.kmax;
        p.k = k;
        p.sweep0 = sweep0 + (uint32_t)done;
        p.src = L->alloc[L->cur] + (size_t)L->ghost * L->pitch;
        p.dst = L->alloc[L->cur ^ 1] + (size_t)L->ghost * L->pitch;
        const int tiles_y = launch_tiles(L, tv, k, n_sweeps - done, part, slab, p);
        const bool quad = quad_fits(L, tv, p.tile_h + 4 * k);  // (after launch_tiles: the tile height is the pair table's)
        void (*const kern)(TiledParams) = quad ? tv.kernel_q : (L->periodic ? tv.kernel : tv.open);
        if (quad) TSU_HIP_TRY(ctx, tsu_func_allow_lds(ctx, (const void*)kern, 160 * 1024));
        const size_t lds_bytes = tile_lds_bytes(tv, p.tile_h + 4 * k, quad);
        if (verbose)
            fprintf(stderr, "[tsu] k1_tiled2 variant %d: %d tile rows of %d, %d sweeps, thresholds: %s\n", c.v, tiles_y, p.tile_h, k,
                    quad ? "quad table" : (L->periodic ? "pair table" : "v_perm"));
        // tile rows 0 and tiles_y-1 read ghost rows (2k <= H); the others only read owned rows
        int n_ty = tiles_y;
        p.ty_first = 0;
        p.ty_stride = 1;
        if (part == TSU_PART_INTERIOR) {
            p.ty_first = 1;
            n_ty = tiles_y - 2;
        } else if (part == TSU_PART_BOUNDARY && tiles_y >= 2) {
            p.ty_stride = tiles_y - 1;
            n_ty = 2;
        }
        if (n_ty > 0) {
            hipLaunchKernelGGL(kern, dim3((unsigned)(p.tiles_x * n_ty)), dim3((unsigned)tv.threads), lds_bytes, ctx->stream, p);
            L->launches += 1;
        }
        if (part != TSU_PART_INTERIOR) L->cur ^= 1;  // INTERIOR does not publish; BOUNDARY (or ALL) does
        done += k;
    }
    TSU_HIP_TRY(ctx, hipGetLastError());
    return TSU_OK;
}
}  // namespace

int tsu_ising2d_tiled_supported(const tsu_ising2d* L) {
    if (plan_call(L, 0, TSU_PART_ALL).v < 0) return 0;       // no tile shape fits (too narrow / too few rows): generic kernel
    const bool open_whole = !L->periodic && L->ghost == 0 && L->total_rows == L->rows;  // beyond its edges: nothing
    if (!L->wrap_rows && !open_whole && L->ghost < 2) return 0;
    return 1;
}

// number of tiles (= workgroups of a tile-resident launch) the lattice is cut into; 0 if the tiled kernel does not apply
int tsu_ising2d_tiled_tiles(const tsu_ising2d* L) {
    if (!tsu_ising2d_tiled_supported(L)) return 0;
    const CallPlan c = plan_call(L, 0, TSU_PART_ALL);
    const TileVariant& tv = kVariants[c.v];
    const int tiles_x = (((L->cols + 15) / 16) + tv.WO - 1) / tv.WO;
    return (c.flex_ty > 0 ? c.flex_ty : (L->rows + tv.H - 1) / tv.H) * tiles_x;
}

// split (interior / boundary) launches: ghost-row slabs whose tile rows are all full
int tsu_ising2d_tiled_part_supported(const tsu_ising2d* L) {
    return tsu_ising2d_tiled_supported(L) && !L->wrap_rows && (L->rows % kVariants[plan_call(L, 0, TSU_PART_ALL).v].H) == 0;
}

int tsu_ising2d_tiled_sweep(tsu_ising2d* L, int n_sweeps, uint64_t seed, uint32_t sweep0, uint32_t replica, int part) {
    tsu_ctx* ctx = L->ctx;
    const CallPlan c = plan_call(L, n_sweeps, part);
    const TileVariant& tv = kVariants[c.v];
    if (!L->alloc[1]) {
        size_t bytes = (size_t)(L->rows + 2 * L->ghost) * L->pitch;
        TSU_HIP_TRY(ctx, hipMalloc(&L->alloc[1], bytes));
        TSU_HIP_TRY(ctx, hipMemsetAsync(L->alloc[1], 0, bytes, ctx->stream));
    }
    if (!L->wrap_rows && !(!L->periodic && L->ghost == 0 && L->total_rows == L->rows)) {
        // A slab may sweep ghost/2 times between two ghost refreshes.  When that takes several launches, every launch
        // but the last also computes the ghost rows the following launches will read (2 rows per remaining sweep on
        // each side, from input that is still exact there), instead of waiting for the neighbours.
        TSU_REQUIRE(ctx, 2 * n_sweeps <= L->ghost, "ising2d_sweep (tiled, slab): %d sweeps per ghost refresh exceed ghost/2 = %d",
                    n_sweeps, L->ghost / 2);
        TSU_REQUIRE(ctx, part == TSU_PART_ALL || n_sweeps <= c.kmax, "ising2d_sweep_part: split sweeps take at most %d sweeps", c.kmax);
    }
    TiledParams p;
    p.pitch = (long long)L->pitch;
    p.rows = L->rows;
    p.nchunks = (L->cols + 15) / 16;
    p.cols = L->cols;
    p.row0 = L->row0;
    p.total_rows = L->total_rows;
    p.wrap_rows = L->wrap_rows;
    p.ghost = L->ghost;
    p.tiles_x = (p.nchunks + tv.WO - 1) / tv.WO;
    p.q_shift = ragged_shift(L, tv.WO);
    p.r_begin = 0;
    p.r_end = L->rows;
    p.tile_h = tv.H;
    p.flex_ty = 0;
    ising2d_set_keys(p, seed, replica);
    pack_thresholds(p, L->table);
    p.open = L->periodic ? 0 : 1;
    TSU_HIP_TRY(ctx, tsu_func_allow_lds(ctx, (const void*)(L->periodic ? tv.kernel : tv.open), 160 * 1024));
    if (c.resident) {
        // the quad kernel first, where its table fits beside the planned tile and the chip still holds every tile; else the planned form
        for (int quad = quad_fits(L, tv, c.tile_h + 4 * c.kmax) ? 1 : 0; quad >= 0; --quad) {
            void (*const res_kern)(ResidentLaunch) = quad ? tv.resident_q : (L->periodic ? tv.resident : tv.resident_open);
            TSU_HIP_TRY(ctx, tsu_func_allow_lds(ctx, (const void*)res_kern, 160 * 1024));
            int fit_per_cu = 0;
            // (occupancy for the standard tile height; a stretched slab tile was checked against the variant's LDS share)
            TSU_HIP_TRY(ctx, tsu_func_blocks_per_cu(ctx, (const void*)res_kern, tv.threads,
                                                    tile_lds_bytes(tv, (c.flex_ty > 0 ? c.tile_h : tv.H) + 4 * KMAX, quad != 0), &fit_per_cu));
            if ((long long)p.tiles_x * c.tiles_y <= (long long)fit_per_cu * ctx->cus) return run_resident(L, c, p, n_sweeps, sweep0, fit_per_cu, quad != 0);
        }
    }
    return run_generations(L, c, p, n_sweeps, sweep0, part);
}

// ================================================================== one-workgroup colour-plane kernel (small lattices)
// A whole lattice of at most 1024 octets (32 x 32 ... 128 x 128: the reference's own sizes, BASELINE configs[0]) as two
// colour planes of up-flags in one workgroup's LDS for all sweeps of a call: one thread per octet, the tiled kernel's
// packed-byte update (one Philox block, 16-bit threshold compare, lazy low bits on ties) with true wrap-around
// indices instead of a halo.  Same counters (octet, row, half-sweep), hence the same results as every other lattice
// kernel.  Workgroup b of a launch sweeps lattice b of a batch (one temperature each of a scan).
struct PlanesItem {
    int8_t* buf;  // owned row 0 (updated in place: the lattice lives in LDS between the load and the store)
    long long pitch;
    int rows, cols, periodic;
    uint32_t k0, k1, tag_hi, tag_lo, sweep0;
    uint32_t tblH0, tblH1, tblL0, tblL1, t3H0, t3H1, t3L0, t3L1;
    uint64_t thr[25];
};

template <bool OPEN>
__global__ __launch_bounds__(1024) void k1_planes(const PlanesItem* __restrict__ items, PlanesItem one, int n_sweeps) {
    __shared__ uint64_t s_planes[2 * 1024];
    __shared__ uint64_t s_thr[25];
    const PlanesItem& it = items ? items[blockIdx.x] : one;
    const int tid = threadIdx.x;
    const int rows = it.rows, cols = it.cols, nch = (cols + 15) >> 4, tasks = rows * nch;
    if (tid < 25) s_thr[tid] = it.thr[tid];
    const PhiloxKeys K = make_keys(it.k0, it.k1);
    const bool active = tid < tasks;
    const int r = active ? tid / nch : 0, q = active ? tid - r * nch : 0;
    const int idx = r * nch + q;
    uint64_t* const plane0 = s_planes;
    uint64_t* const plane1 = s_planes + tasks;
    // the columns of this chunk that exist (open lattices of ragged width: fewer in the last chunk)
    int nv = cols - 16 * q;
    if (nv > 16) nv = 16;
    auto first_sites = [](int n) { return n >= 8 ? 0x0101010101010101ull : (((1ull << (8 * n)) - 1) & 0x0101010101010101ull); };
    const uint64_t vm_e = first_sites((nv + 1) >> 1), vm_o = first_sites(nv >> 1);
    int8_t* const chunk = it.buf + (long long)r * it.pitch + 16 * q;
    if (active) {
        const uint4 v = *reinterpret_cast<const uint4*>(chunk);
        const uint32_t e0 = perm(v.y, v.x, 0x06040200u), e1 = perm(v.w, v.z, 0x06040200u);
        const uint32_t o0 = perm(v.y, v.x, 0x07050301u), o1 = perm(v.w, v.z, 0x07050301u);
        uint64_t ev = (uint64_t)(~(e0 >> 1) & 0x01010101u) | ((uint64_t)(~(e1 >> 1) & 0x01010101u) << 32);
        uint64_t od = (uint64_t)(~(o0 >> 1) & 0x01010101u) | ((uint64_t)(~(o1 >> 1) & 0x01010101u) << 32);
        ev &= vm_e;  // the row's pad bytes are 0, which would read as "up"
        od &= vm_o;
        ((r & 1) ? plane1 : plane0)[idx] = ev;  // the even columns of row r have colour r & 1
        ((r & 1) ? plane0 : plane1)[idx] = od;
    }
    // neighbour octets: -1 = beyond an open edge (nothing there)
    const int up = r > 0 ? idx - nch : (OPEN ? -1 : idx + (rows - 1) * nch);
    const int dn = r < rows - 1 ? idx + nch : (OPEN ? -1 : idx - (rows - 1) * nch);
    const int lf = q > 0 ? idx - 1 : (OPEN ? -1 : idx + nch - 1);
    const int rt = q < nch - 1 ? idx + 1 : (OPEN ? -1 : idx - (nch - 1));
    // a periodic lattice of ragged width wraps inside the last octet: the site after its last valid one (v_last - 1) is
    // site 0 of octet 0, the site before site 0 of octet 0 is that last valid one
    const int v_last = ((cols >> 1) & 7) ? ((cols >> 1) & 7) : 8;
    const int shl = q == nch - 1 ? 8 * (v_last - 1) : 56, shr = q == 0 ? 8 * (v_last - 1) : 56;
    Rows2Ctx c;
    c.s_thr = s_thr;
    c.t3H0 = it.t3H0; c.t3H1 = it.t3H1; c.t3L0 = it.t3L0; c.t3L1 = it.t3L1;
    asm volatile("v_mov_b32 %0, %1" : "=v"(c.tblH0) : "s"(it.tblH0));
    asm volatile("v_mov_b32 %0, %1" : "=v"(c.tblH1) : "s"(it.tblH1));
    asm volatile("v_mov_b32 %0, %1" : "=v"(c.tblL0) : "s"(it.tblL0));
    asm volatile("v_mov_b32 %0, %1" : "=v"(c.tblL1) : "s"(it.tblL1));
    c.r_par = (uint32_t)(cols - 1) & 1u;
    c.r_slot = ((uint32_t)(cols - 1) & 15u) >> 1;
    c.rm_lo = c.r_slot < 4 ? 0xFFu << (8 * c.r_slot) : 0u;
    c.rm_hi = c.r_slot < 4 ? 0u : 0xFFu << (8 * (c.r_slot - 4));
    const bool row_edge = OPEN && (r == 0 || r == rows - 1);
    const uint32_t tag_hi = it.tag_hi, tag_lo = it.tag_lo, k0 = it.k0, k1 = it.k1, sweep0 = it.sweep0;
    for (int hsi = 0; hsi < 2 * n_sweeps; ++hsi) {
        __syncthreads();
        const int kappa = hsi & 1;
        const uint32_t hs = 2u * (sweep0 + (uint32_t)(hsi >> 1)) + (uint32_t)kappa;
        if (active) {
            const uint64_t* Ps = kappa ? plane0 : plane1;
            uint64_t* Pd = kappa ? plane1 : plane0;
            const int par = (r + kappa) & 1;  // column parity of the sites updated in this row
            const uint64_t U = (OPEN && up < 0) ? 0ull : Ps[up], D = (OPEN && dn < 0) ? 0ull : Ps[dn], C = Ps[idx];
            // horizontal neighbours: compact bytes (j, j+1) when the parity is 1, (j-1, j) when it is 0
            const int side = par ? rt : lf;
            const uint64_t A = (OPEN && side < 0) ? 0ull : Ps[side];
            const uint64_t S = par ? ((C >> 8) | ((A & 0xFFull) << shl)) : ((C << 8) | ((A >> shr) & 0xFFull));
            const uint64_t cnt = U + D + C + S;  // bytes <= 4: no carries between sites
            const uint32_t cnt_lo = (uint32_t)cnt, cnt_hi = (uint32_t)(cnt >> 32);
            const u32x4 w = philox_vk((uint32_t)q, (uint32_t)r, 0xFFFFFFFFu, philox_y0(hs, k0), hs, tag_hi, K);
            u32x4 d;
            uint32_t edge = 0;
            if (OPEN) {
                const bool l0 = !par && q == 0, r7 = q == nch - 1 && c.r_par == (uint32_t)par;
                d = compare_octet_open(w, cnt_lo, cnt_hi, c, row_edge, l0, r7);
                edge = (row_edge ? 1u : 0u) | (l0 ? 2u : 0u) | (r7 ? 4u : 0u) | (c.r_slot << 4);
            } else {
                d = compare_octet(w, cnt_lo, cnt_hi, c.tblH0, c.tblH1, c.tblL0, c.tblL1);
            }
            if (__builtin_expect(has_zero_field(d), 0)) d = resolve_ties(d, w, cnt_lo, cnt_hi, s_thr, (uint32_t)q, (uint32_t)r, hs, tag_lo, k0, k1, edge);
            uint64_t n = pack_flags(d);
            n &= par ? vm_o : vm_e;
            Pd[idx] = n;
        }
    }
    __syncthreads();
    if (active) {
        const uint64_t ev = ((r & 1) ? plane1 : plane0)[idx], od = ((r & 1) ? plane0 : plane1)[idx];
        const uint32_t e0 = perm(0u, 0x000001FFu, (uint32_t)ev), e1 = perm(0u, 0x000001FFu, (uint32_t)(ev >> 32));
        const uint32_t o0 = perm(0u, 0x000001FFu, (uint32_t)od), o1 = perm(0u, 0x000001FFu, (uint32_t)(od >> 32));
        uint4 v = make_uint4(perm(o0, e0, 0x05010400u), perm(o0, e0, 0x07030602u), perm(o1, e1, 0x05010400u), perm(o1, e1, 0x07030602u));
        if (nv < 16) {  // ragged last chunk: the pad bytes of the row stay 0
            auto bytes = [](int n) { return n >= 4 ? 0xFFFFFFFFu : (n <= 0 ? 0u : (1u << (8 * n)) - 1u); };
            v.x &= bytes(nv);
            v.y &= bytes(nv - 4);
            v.z &= bytes(nv - 8);
            v.w &= bytes(nv - 12);
        }
        *reinterpret_cast<uint4*>(chunk) = v;
    }
}

// whole lattices of at most 1024 octets, any width; a lattice needs two rows and two columns (the packed compare knows
// degrees 4, 3 and 2): one-row and one-column lattices take k1_generic
int tsu_ising2d_planes_supported(const tsu_ising2d* L) {
    if (L->ghost != 0 || L->total_rows != L->rows || L->row0 != 0) return 0;
    if ((long long)L->rows * ((L->cols + 15) / 16) > 1024) return 0;
    return L->rows >= 2 && L->cols >= 2;
}

// one launch for n lattices of one shape and boundary (workgroup b sweeps lattice b); caller checked planes_supported
int tsu_ising2d_planes_sweep(tsu_ising2d* const* lats, int n, int n_sweeps, const uint64_t* seeds, const uint32_t* sweep0s,
                             const uint32_t* replicas) {
    tsu_ctx* ctx = lats[0]->ctx;
    std::vector<PlanesItem> items((size_t)n);
    for (int i = 0; i < n; ++i) {
        const tsu_ising2d* L = lats[i];
        PlanesItem& it = items[(size_t)i];
        it.buf = L->alloc[L->cur] + (size_t)L->ghost * L->pitch;
        it.pitch = (long long)L->pitch;
        it.rows = L->rows;
        it.cols = L->cols;
        it.periodic = L->periodic;
        ising2d_set_keys(it, seeds[i], replicas[i]);
        it.sweep0 = sweep0s[i];
        pack_thresholds(it, L->table);
    }
    const tsu_ising2d* L0c = lats[0];
    const int tasks = L0c->rows * ((L0c->cols + 15) / 16);
    const unsigned threads = (unsigned)((tasks + 63) / 64 * 64);
    void (*const kern)(const PlanesItem*, PlanesItem, int) = L0c->periodic ? k1_planes<false> : k1_planes<true>;
    if (n == 1) {
        hipLaunchKernelGGL(kern, dim3(1), dim3(threads), 0, ctx->stream, (const PlanesItem*)nullptr, items[0], n_sweeps);
    } else {
        tsu_ising2d* L0 = lats[0];  // the staging buffer for the items lives with the first lattice of the batch
        const size_t bytes = items.size() * sizeof(PlanesItem);
        TSU_HIP_TRY(ctx, ising2d_grow(L0->d_batch, L0->batch_cap, bytes));
        // stream order keeps a previous batch launch from still reading the buffer; the host array dies with this call,
        // so the copy is waited for (a few KB); the launch itself stays asynchronous
        TSU_HIP_TRY(ctx, hipMemcpyAsync(L0->d_batch, items.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
        TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        hipLaunchKernelGGL(kern, dim3((unsigned)n), dim3(threads), 0, ctx->stream, (const PlanesItem*)L0->d_batch, items[0], n_sweeps);
    }
    TSU_HIP_TRY(ctx, hipGetLastError());
    for (int i = 0; i < n; ++i) lats[i]->launches += 1;
    return TSU_OK;
}

// sparse_host.h -- the host side of K5's route choice (sparse.hip): validation of a coloured CSR graph, its position-space form, the
// classifier of REGULAR colour classes, the pairing pass and the launch rule of the four-positions-per-thread kernels.  Plain C++ with
// no HIP includes: tsu_sparse_create runs it before it uploads anything, tsu_sparse_classify runs it without a context or a GPU, and
// a test can ask either which kernel a colour class takes (k5_plan_record).  Internal linkage throughout.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

// A REGULAR colour class (chains, rings, ladders ...: `IsingChain`, tsu/models/ising.py:265-286): apart from at most K5_EDGE rows at
// either end of its position range, every row has the same degree, the same coupling on every edge, the same bias, neighbours at
// fixed position offsets and a site number that is affine in the position.  Such a class needs no CSR streams at all: per update it
// reads its neighbours' bits (deg bytes, contiguous across the lanes) and writes one byte -- ~3 B instead of 43 for a chain -- and
// the field takes deg + 1 values only, so acceptance is one integer compare of the uniform's 53 bits with a threshold computed (on
// the device, with the generic kernel's own expressions) from the number of set neighbours.  The end rows run on the generic kernel.
#define K5_MAX_DEG 4
#define K5_EDGE 64
struct K5Stencil {
    int deg;            // -1: not regular
    int pb, pe;         // position range of the class
    int lo, hi;         // rows [pb, pb + lo) and [pe - hi, pe) are irregular (generic kernel)
    int off[K5_MAX_DEG];
    double Jv, bias;
    int site0, site_stride;  // site of position p = site0 + site_stride * (p - pb - lo)
    // PAIRED classes.  The uniform of site i comes from the Philox block of i >> 1 (dense.h: words x, y for the even site, z, w for the
    // odd one), and in a chain the two sites of a block sit in the two colour classes at the same index: the launch of the first class
    // (pair = 1) has the second class's uniform in registers for free.  It cannot decide for that site yet -- its neighbours are being
    // updated -- but the decision is a function of the neighbour count alone: bit k of code[p'] = "the site at position p' of the other
    // class becomes 1 if k of its neighbours are set".  The second class's launch (pair = 2, k5_paired) computes no random numbers
    // at all: count, shift, store.  Philox blocks per sweep: one per PAIR of sites instead of one per site.
    int pair;                // 0: none; 1: prepares the codes of class `other`; 2: consumes them
    int other;               // the partner class
    int o_pb, o_lo, o_n;     // (pair = 1) the partner's first position, its leading irregular rows and the number of its REGULAR rows
    int o_deg;
};

// graphs of at most this many sites run whole on k5_small (one workgroup, the state in LDS), whatever their classes look like
constexpr int K5S_MAX = 32768;

// an environment switch that is ON unless set to 0
static inline bool k5_env_on(const char* name) {
    const char* v = getenv(name);
    return !(v && atoi(v) == 0);
}

// what tsu_sparse_create derives on the host
struct K5Host {
    std::vector<int32_t> pos_of;     // site -> position
    std::vector<int64_t> rp;         // position-space CSR
    std::vector<int32_t> cp;
    std::vector<double> vp, bp;
    std::vector<K5Stencil> stencil;  // one per colour; deg < 0: the class is not regular
    bool any_pair;
};

#define K5_HOST_REQUIRE(cond, ...)            \
    do {                                      \
        if (!(cond)) {                        \
            snprintf(err, err_n, __VA_ARGS__); \
            return false;                     \
        }                                     \
    } while (0)

// validate: CSR arrays and offsets sane, order is a permutation, rows ascending and in range, the colouring is proper.  Fills pos_of.
// false: `err` holds the message (prefixed with `who`, the entry point's name)
static inline bool k5_host_validate(const char* who, int n, const int64_t* row_ptr, const int32_t* col_idx, const double* values, int n_colors,
                                    const int32_t* color_offsets, const int32_t* order, std::vector<int32_t>& pos_of, char* err, size_t err_n) {
    K5_HOST_REQUIRE(n > 0 && row_ptr && n_colors > 0 && color_offsets && order, "%s: bad arguments", who);
    const int64_t nnz = row_ptr[n];
    K5_HOST_REQUIRE(row_ptr[0] == 0 && nnz >= 0 && (nnz == 0 || (col_idx && values)), "%s: bad CSR arrays", who);
    K5_HOST_REQUIRE(color_offsets[0] == 0 && color_offsets[n_colors] == n, "%s: colour offsets must run from 0 to n", who);
    pos_of.assign((size_t)n, -1);
    std::vector<int32_t> color_of((size_t)n, -1);
    for (int c = 0; c < n_colors; ++c) {
        K5_HOST_REQUIRE(color_offsets[c] <= color_offsets[c + 1], "%s: colour offsets must not decrease", who);
        for (int p = color_offsets[c]; p < color_offsets[c + 1]; ++p) {
            const int32_t i = order[p];
            K5_HOST_REQUIRE(i >= 0 && i < n && pos_of[(size_t)i] < 0, "%s: order is not a permutation of 0..n-1", who);
            pos_of[(size_t)i] = p;
            color_of[(size_t)i] = c;
        }
    }
    for (int i = 0; i < n; ++i) {
        K5_HOST_REQUIRE(row_ptr[i] <= row_ptr[i + 1], "%s: row_ptr must not decrease", who);
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            const int32_t j = col_idx[e];
            K5_HOST_REQUIRE(j >= 0 && j < n, "%s: column index out of range", who);
            K5_HOST_REQUIRE(e == row_ptr[i] || col_idx[e - 1] < j, "%s: columns of a row must ascend", who);
            K5_HOST_REQUIRE(j == i || color_of[(size_t)j] != color_of[(size_t)i], "%s: sites %d and %d are coupled but have the same colour", who, i,
                            (int)j);
        }
    }
    return true;
}

// the position-space CSR of a validated graph: row p is the row of site order[p], its columns are the neighbours' POSITIONS (in
// ascending order of the neighbours' site numbers)
static inline void k5_host_position_csr(int n, const int64_t* row_ptr, const int32_t* col_idx, const double* values, const double* bias_host,
                                        const int32_t* order, K5Host& H) {
    const int64_t nnz = row_ptr[n];
    H.rp.assign((size_t)n + 1, 0);
    H.cp.assign((size_t)nnz, 0);
    H.vp.assign((size_t)nnz, 0.0);
    H.bp.assign((size_t)n, 0.0);
    for (int p = 0; p < n; ++p) {
        const int i = order[p];
        int64_t w = H.rp[(size_t)p];
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e, ++w) {
            H.cp[(size_t)w] = H.pos_of[(size_t)col_idx[e]];
            H.vp[(size_t)w] = values[e];
        }
        H.rp[(size_t)p + 1] = w;
        if (bias_host) H.bp[(size_t)p] = bias_host[i];
    }
}

// regular colour classes: the pattern of the class's middle row must hold for every row but at most K5_EDGE at either end
static inline void k5_host_classify(int n_colors, const int32_t* color_offsets, const int32_t* order, bool use_stencil, K5Host& H) {
    const std::vector<int64_t>& rp = H.rp;
    const std::vector<int32_t>& cp = H.cp;
    const std::vector<double>&vp = H.vp, &bp = H.bp;
    H.stencil.assign((size_t)n_colors, K5Stencil());
    for (int c = 0; c < n_colors; ++c) {
        K5Stencil& S = H.stencil[(size_t)c];
        S.deg = -1;
        const int pb = color_offsets[c], pe = color_offsets[c + 1];
        if (!use_stencil || pe - pb < 4 * K5_EDGE + 2) continue;
        const int pm = pb + (pe - pb) / 2;
        const int deg = (int)(rp[(size_t)pm + 1] - rp[(size_t)pm]);
        if (deg < 1 || deg > K5_MAX_DEG) continue;
        K5Stencil T;
        T.deg = deg;
        T.pb = pb;
        T.pe = pe;
        T.Jv = vp[(size_t)rp[(size_t)pm]];
        T.bias = bp[(size_t)pm];
        for (int i = 0; i < K5_MAX_DEG; ++i) T.off[i] = i < deg ? cp[(size_t)rp[(size_t)pm] + i] - pm : 0;
        T.site_stride = order[pm + 1] - order[pm];
        auto fits = [&](int p) {
            if (rp[(size_t)p + 1] - rp[(size_t)p] != deg || bp[(size_t)p] != T.bias) return false;
            if ((long long)order[p] != (long long)order[pm] + (long long)T.site_stride * (p - pm)) return false;
            for (int i = 0; i < deg; ++i) {
                const int64_t e = rp[(size_t)p] + i;
                if (vp[(size_t)e] != T.Jv || cp[(size_t)e] - p != T.off[i] || cp[(size_t)e] == p) return false;  // (no self-loops: the row's own bit is rewritten)
            }
            return true;
        };
        int lo = 0, hi = 0;
        while (lo <= K5_EDGE && !fits(pb + lo)) ++lo;
        while (hi <= K5_EDGE && !fits(pe - 1 - hi)) ++hi;
        if (lo > K5_EDGE || hi > K5_EDGE) continue;
        bool ok = true;
        for (int p = pb + lo; p < pe - hi && ok; ++p) ok = fits(p);
        if (!ok) continue;
        T.lo = lo;
        T.hi = hi;
        T.site0 = order[pb + lo];
        T.pair = 0;
        T.other = -1;
        T.o_pb = T.o_lo = T.o_n = T.o_deg = 0;
        S = T;
    }
}

// pairs of regular classes that share their Philox blocks index by index (K5Stencil::pair): sites ascending by 2 over the WHOLE
// class (end rows included), the first sites of the two classes are the two sites of one block, and every regular row of the
// second class has its partner in the first
static inline void k5_host_pair(int n_colors, const int32_t* order, bool use_pairs, K5Host& H) {
    H.any_pair = false;
    for (int c = 0; c < n_colors && use_pairs; ++c) {
        K5Stencil& A = H.stencil[(size_t)c];
        if (A.deg <= 0 || A.pair || A.site_stride != 2) continue;
        for (int c2 = c + 1; c2 < n_colors; ++c2) {
            K5Stencil& B = H.stencil[(size_t)c2];
            if (B.deg <= 0 || B.pair || B.site_stride != 2) continue;
            if ((order[A.pb] ^ 1) != order[B.pb]) continue;
            bool ok = true;
            for (int q = A.pb; q < A.pe && ok; ++q) ok = order[q] == order[A.pb] + 2 * (q - A.pb);
            for (int q = B.pb; q < B.pe && ok; ++q) ok = order[q] == order[B.pb] + 2 * (q - B.pb);
            if (!ok || (B.pe - B.hi) - B.pb > A.pe - A.pb) continue;  // (a regular row of B beyond A's last index would have no code)
            A.pair = 1;
            A.other = c2;
            A.o_pb = B.pb;
            A.o_lo = B.lo;
            A.o_n = (B.pe - B.hi) - (B.pb + B.lo);
            A.o_deg = B.deg;
            B.pair = 2;
            B.other = c;
            H.any_pair = true;
            break;
        }
    }
}

// validation, position-space CSR, classifier and pairing in the order tsu_sparse_create needs them; the switches TSU_K5_STENCIL and
// TSU_K5_PAIR are read here, i.e. when the handle is created (or a graph classified)
static inline bool k5_host_prepare(const char* who, int n, const int64_t* row_ptr, const int32_t* col_idx, const double* values,
                                   const double* bias_host, int n_colors, const int32_t* color_offsets, const int32_t* order, K5Host& H, char* err,
                                   size_t err_n) {
    if (!k5_host_validate(who, n, row_ptr, col_idx, values, n_colors, color_offsets, order, H.pos_of, err, err_n)) return false;
    k5_host_position_csr(n, row_ptr, col_idx, values, bias_host, order, H);
    k5_host_classify(n_colors, color_offsets, order, k5_env_on("TSU_K5_STENCIL"), H);
    k5_host_pair(n_colors, order, k5_env_on("TSU_K5_PAIR"), H);
    return true;
}

// The launch rule of a regular class: four positions per thread (k5_stencil4) when the class's first position -- and, for the first
// class of a pair, the partner's: the codes leave as dwords -- is a multiple of 4; one position per thread (k5_stencil1) otherwise.
// use_v4: the switch TSU_K5_V4, read by the caller at the time of the launch.
static inline bool k5_launch_v4(bool use_v4, int pb, int pair, int o_pb) { return use_v4 && pb % 4 == 0 && (pair != 1 || o_pb % 4 == 0); }

// The PLAN of a colour class, ten int32 (tsu_sparse_classify / tsu_sparse_class_plan, include/tsu_hip.h):
// route (0: k5_color, 1: k5_stencil1 / k5_stencil4, 2: the whole system on k5_small), deg, lo, hi, site_stride, pair, other, v4, o_lo, o_n.
// A class that is not regular has no stencil: its other fields are 0 and `other` is -1.  Route 2 keeps what the classifier found for
// the class (tsu_sparse_create classifies whatever n is) with v4 = 0: no stencil kernel is launched.
#define K5_PLAN_LEN 10
static inline void k5_plan_record(int n, const K5Stencil& S, bool use_v4, int32_t rec[K5_PLAN_LEN]) {
    for (int i = 0; i < K5_PLAN_LEN; ++i) rec[i] = 0;
    rec[6] = -1;
    const bool small = n <= K5S_MAX;
    rec[0] = small ? 2 : S.deg > 0 ? 1 : 0;
    if (S.deg <= 0) return;
    rec[1] = S.deg;
    rec[2] = S.lo;
    rec[3] = S.hi;
    rec[4] = S.site_stride;
    rec[5] = S.pair;
    rec[6] = S.pair ? S.other : -1;
    rec[7] = !small && k5_launch_v4(use_v4, S.pb, S.pair, S.o_pb) ? 1 : 0;
    rec[8] = S.pair == 1 ? S.o_lo : 0;
    rec[9] = S.pair == 1 ? S.o_n : 0;
}

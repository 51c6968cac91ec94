// multispin_quench.hip -- K9: real-space correlations of the overlap field, two-time correlations against snapshots, and quench
// runs that record both beside the measurements, 64 samples at once (gfx950).
//
// The site field is f = a b, the two replicas of a slot, or f = s with one replica (include/tsu_hip_multispin_quench.h, DESIGN.md
// section 3 "Real-space correlations and quench runs of multispin-coded glasses (K9)").  With X = a ^ b (or X = a) the correlator
// of a periodic axis d is C_d[r] = N - 2 count(bits set in X_x ^ X_{x + r e_d}) per bit position, r = 0 .. L_d / 2: a positional
// popcount over N (L_d / 2 + 1) word pairs.  The kernels keep the counts, the host subtracts.
//
// k9_c4: one launch for all (slot, word-plane) pairs (the grid's y) and all periodic axes (the grid's z).  A workgroup takes a
// bundle of lines along its axis and stages X of them in LDS, every word of a and b read once from HBM per axis: for the column axis
// the bundle is a run of whole rows, for the row and layer axes slabs of 16 consecutive columns x the full axis (narrower only
// where 16 columns of a long axis exceed the LDS), so the global loads stay 128-byte runs; in LDS a line is contiguous whatever its
// axis (stride L + 1 words).  Then a lane owns one displacement r of one line and walks x = 0 .. L - 1 reading X[x] (the same
// address in all lanes of the line: a broadcast) and X[(x + r) mod L] (consecutive lanes, consecutive 8-byte words: every bank once
// per 32 lanes).  With D = L / 2 + 1 < 64 displacements a wave takes 64 / D lines side by side; with D > 64 the displacements are
// cut into blocks of 64 that the workgroup takes one after the other over the same staged lines.  A lane adds its one-bit words
// into an 8-plane vertical counter (MscCount<8>), three at a time through one carry-save step (sum at weight 1, carry at weight 2:
// the same counter value for fewer ripple steps), and flushes it before its 256th addition into the workgroup's LDS counters
// [r][bit]; after a block the workgroup adds those to the row with 32-bit integer vector atomics (the row was zeroed by a memset;
// a count is at most N <= 2^30).  No floating point, no scratch memory, no waiting on other workgroups.
//
// k9_twotime: the set bits of now ^ snapshot per plane and bit position, one launch for all planes of one snapshot: k9_measure's
// shape (vertical counters of at most 32 additions, LDS counters, integer atomics into a zeroed row).
//
// A quench run (tsu_msc_quench_run) strings sweeps (msc_enqueue_sweeps: the handle's own route), k9_measure, k9_c4, snapshot copies
// and k9_twotime on the handle's stream into a device record; tsu_msc_quench_history fetches it.
#include <new>
#include <vector>

#include "multispin_host.h"

namespace {

constexpr int kC4Lanes = 256;
constexpr int kC4Block = 64;                 // displacements of a block: one per lane of a wave
constexpr int kC4AccWords = kC4Block * 64;   // LDS counters of a workgroup: [displacement of the block][bit]
constexpr int kC4Adds = 255;                 // additions of a lane between two flushes: 2^8 - 1, the most 8 planes hold
constexpr int kC4TargetWords = 4096;         // words of X a bundle aims at (32 KiB)
constexpr int kC4MaxWords = 16384;           // words of X a bundle may hold: 128 KiB beside 16 KiB of counters
constexpr int kC4Slab = 16;                  // columns of a slab: 128 bytes
constexpr int kTTSites = 32;                 // sites per lane of k9_twotime: one addition each into 6-plane counters (at most 63)

struct MscC4Axis {
    int d;        // 0 layers, 1 rows, 2 columns
    int L, D;     // the axis's length, displacements 0 .. L / 2
    int sw;       // columns of a slab (d < 2), a power of two; 1 for d == 2
    int ncb;      // column blocks of a row: ceil(cols / sw)
    int nunits;   // units of a plane: rows (d == 2) or slabs
    int per;      // units of a bundle
    int nb;       // bundles
    int G, npw;   // lanes of a line: min(D, 64); lines a wave takes side by side: 64 / G
    long long off;  // where the axis's [64 W n_temps][D] block starts in a row
};

struct MscC4 {
    const uint64_t* s;
    int32_t* out;
    int rows, cols, nsites, W;
    MscC4Axis ax[3];
};

// a lane's counter added into its displacement's LDS counters; lanes start at different bits, so a wave's adds spread over the banks
__device__ __forceinline__ void msc_c4_flush(const MscCount<8>& cnt, uint32_t* row, int lane) {
    for (int k = 0; k < 64; ++k) {
        const int bit = (k + lane) & 63;
        const uint32_t v = cnt.value(bit);
        if (v) atomicAdd(row + bit, v);
    }
}

// 2 x added to the counter: the ripple starts at the second plane
__device__ __forceinline__ void msc_c4_add2(MscCount<8>& cnt, uint64_t x) {
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        const uint64_t t = cnt.b[k] & x;
        cnt.b[k] ^= x;
        x = t;
    }
}

template <int A>
__global__ __launch_bounds__(kC4Lanes) void k9_c4(MscC4 p) {
    extern __shared__ __align__(16) uint64_t lds[];
    uint32_t* acc = reinterpret_cast<uint32_t*>(lds);  // kC4AccWords
    uint64_t* X = lds + kC4AccWords / 2;               // lines of L + 1 words
    const MscC4Axis a = p.ax[blockIdx.z];
    if ((int)blockIdx.x >= a.nb) return;
    const int tid = threadIdx.x;
    const int L = a.L, Lp = L + 1, D = a.D, d = a.d, sw = a.sw;
    const int t = blockIdx.y / p.W, w = blockIdx.y - t * p.W;
    const uint64_t* sa = p.s + (long long)((t * A) * p.W + w) * p.nsites;
    const uint64_t* sb = p.s + (long long)((t * A + A - 1) * p.W + w) * p.nsites;
    const int u0 = blockIdx.x * a.per;
    const int nu = min(a.per, a.nunits - u0);
    const int nl = nu * sw;  // lines in LDS
    if (d == 2) {
        const int n = nu * L, first = u0 * L;  // whole rows: one contiguous run of words
        for (int idx = tid; idx < n; idx += kC4Lanes) {
            const int li = idx / L, x = idx - li * L;
            uint64_t v = sa[first + idx];
            if constexpr (A == 2) v ^= sb[first + idx];
            X[li * Lp + x] = v;
        }
    } else {
        const int n = nl * L;
        for (int idx = tid; idx < n; idx += kC4Lanes) {
            const int j = idx & (sw - 1), q = idx / sw;
            const int sl = q / L, x = q - sl * L;
            const int unit = u0 + sl, outer = unit / a.ncb, c = (unit - outer * a.ncb) * sw + j;
            if (c < p.cols) {
                const int i = d == 1 ? (outer * p.rows + x) * p.cols + c : (x * p.rows + outer) * p.cols + c;
                uint64_t v = sa[i];
                if constexpr (A == 2) v ^= sb[i];
                X[(sl * sw + j) * Lp + x] = v;
            }
        }
    }
    const int lane = tid & 63;
    const int lsub = lane / a.G, rl = lane - lsub * a.G;
    const int slot = (tid >> 6) * a.npw + lsub, nslots = (kC4Lanes / 64) * a.npw;
    const long long col0 = (long long)blockIdx.y * 64;
    for (int r0 = 0; r0 < D; r0 += kC4Block) {
        __syncthreads();  // the lines are staged; the last block's counters are out
        for (int k = tid; k < kC4AccWords; k += kC4Lanes) acc[k] = 0;
        __syncthreads();
        const int r = r0 + rl;
        if (lsub < a.npw && r < D) {
            MscCount<8> cnt;
            cnt.clear();
            int adds = 0;
            for (int li = slot; li < nl; li += nslots) {
                if (d != 2) {  // a column past the row's end holds no line
                    const int sl = li / sw, unit = u0 + sl;
                    if ((unit % a.ncb) * sw + (li - sl * sw) >= p.cols) continue;
                }
                const uint64_t* line = X + li * Lp;
                int xr = r;  // r <= L / 2 < L
                int x = 0;
                // three words at a time through a carry-save step: their sum bit enters the counter at weight 1 and their carry at
                // weight 2, 15 ripple steps for what three plain additions do in 24; the counter holds the same value
                for (; x + 3 <= L; x += 3) {
                    if (adds > kC4Adds - 3) {
                        msc_c4_flush(cnt, acc + rl * 64, lane);
                        cnt.clear();
                        adds = 0;
                    }
                    const uint64_t w0 = line[x] ^ line[xr];
                    xr = xr + 1 == L ? 0 : xr + 1;
                    const uint64_t w1 = line[x + 1] ^ line[xr];
                    xr = xr + 1 == L ? 0 : xr + 1;
                    const uint64_t w2 = line[x + 2] ^ line[xr];
                    xr = xr + 1 == L ? 0 : xr + 1;
                    uint64_t sum, carry;
                    msc_full_add(w0, w1, w2, sum, carry);
                    cnt.add(sum);
                    msc_c4_add2(cnt, carry);
                    adds += 3;
                }
                for (; x < L; ++x) {
                    if (adds == kC4Adds) {
                        msc_c4_flush(cnt, acc + rl * 64, lane);
                        cnt.clear();
                        adds = 0;
                    }
                    cnt.add(line[x] ^ line[xr]);
                    ++adds;
                    xr = xr + 1 == L ? 0 : xr + 1;
                }
            }
            msc_c4_flush(cnt, acc + rl * 64, lane);
        }
        __syncthreads();
        const int nr = min(kC4Block, D - r0);
        for (int k = tid; k < kC4AccWords; k += kC4Lanes) {
            const int bit = k >> 6, rr = k & 63;
            if (rr >= nr) continue;
            const uint32_t v = acc[rr * 64 + bit];
            if (v) atomicAdd(p.out + a.off + (col0 + bit) * D + r0 + rr, (int32_t)v);
        }
    }
}

struct MscTT {
    const uint64_t* now;
    const uint64_t* snap;
    int32_t* out;  // [plane][64]
    int nsites;
};

__global__ __launch_bounds__(256) void k9_twotime(MscTT p) {
    __shared__ uint32_t acc[64];
    const int tid = threadIdx.x, plane = blockIdx.y;
    if (tid < 64) acc[tid] = 0;
    __syncthreads();
    const uint64_t* now = p.now + (long long)plane * p.nsites;
    const uint64_t* snap = p.snap + (long long)plane * p.nsites;
    MscCount<6> cnt;
    cnt.clear();
    bool any = false;
    for (int k = 0; k < kTTSites; ++k) {
        const long long i = ((long long)blockIdx.x * kTTSites + k) * 256 + tid;
        if (i >= p.nsites) break;
        any = true;
        cnt.add(now[i] ^ snap[i]);
    }
    if (any) {
        const int lane = tid & 63;
        for (int k = 0; k < 64; ++k) {
            const int bit = (k + lane) & 63;
            const uint32_t v = cnt.value(bit);
            if (v) atomicAdd(&acc[bit], v);
        }
    }
    __syncthreads();
    if (tid < 64 && acc[tid]) atomicAdd(p.out + (long long)plane * 64 + tid, (int32_t)acc[tid]);
}

}  // namespace

struct msc_quench {
    MscC4 plan;            // k9_c4's parameters but for the row
    int naxes;             // periodic axes
    int axis_of[3];        // plan.ax index of axis d, or -1
    size_t lds;            // k9_c4's dynamic LDS
    size_t c4_len;         // int32 entries of a C4 row
    int32_t* d_c4;         // tsu_msc_c4's own row
    int32_t* d_tt;         // tsu_msc_snapshot_overlap's own row
    uint64_t* d_snap;      // n_slots copies of all planes
    int n_slots;
    unsigned taken;        // bit j: slot j holds a snapshot
    // the record of the last quench run
    unsigned long long* d_meas;
    int32_t* d_c4h;
    int32_t* d_tth;
    size_t meas_cap, c4h_cap, tth_cap;  // bytes
    int n_times, n_wait;
    int wait_index[TSU_MSC_SNAPSHOT_SLOTS];
};

namespace {

inline size_t msc_q_cols(const tsu_msc* h) { return (size_t)h->nT * h->W * 64; }
inline size_t msc_q_tt_len(const tsu_msc* h) { return msc_planes(h) * 64; }
inline size_t msc_q_plane_words(const tsu_msc* h) { return msc_planes(h) * (size_t)h->g.nsites; }

// the handle's quench state with k9_c4's launch plan, made on first use
int msc_quench_state(tsu_msc* h, const char* who) {
    tsu_ctx* ctx = h->ctx;
    if (h->qn) return TSU_OK;
    msc_quench* q = new (std::nothrow) msc_quench();
    if (!q) return tsu_fail(ctx, TSU_E_NOMEM, "%s: host allocation failed", who);
    const int len[3] = {h->g.depth, h->g.rows, h->g.cols};
    const int per[3] = {h->g.pz, h->g.pr, h->g.pc};
    q->plan.s = h->d_s;
    q->plan.rows = h->g.rows;
    q->plan.cols = h->g.cols;
    q->plan.nsites = h->g.nsites;
    q->plan.W = h->W;
    long long off = 0;
    for (int d = 0; d < 3; ++d) {
        q->axis_of[d] = -1;
        if (!per[d] || len[d] > TSU_MSC_C4_MAX_AXIS) continue;  // too long an axis: tsu_msc_c4 refuses the handle
        MscC4Axis& a = q->plan.ax[q->naxes];
        q->axis_of[d] = q->naxes++;
        a.d = d;
        a.L = len[d];
        a.D = len[d] / 2 + 1;
        a.G = a.D < 64 ? a.D : 64;
        a.npw = 64 / a.G;
        const int Lp = a.L + 1;
        if (d == 2) {
            a.sw = 1;
            a.ncb = 1;
            a.nunits = h->g.depth * h->g.rows;
        } else {
            a.sw = kC4Slab;
            while (a.sw > 1 && (a.sw * Lp > kC4MaxWords || a.sw / 2 >= h->g.cols)) a.sw /= 2;
            a.ncb = (h->g.cols + a.sw - 1) / a.sw;
            a.nunits = (d == 1 ? h->g.depth : h->g.rows) * a.ncb;
        }
        const int unit_words = a.sw * Lp;  // <= kC4MaxWords: L + 1 <= TSU_MSC_C4_MAX_AXIS + 1
        a.per = kC4TargetWords / unit_words;
        if (a.per < 1) a.per = 1;
        if (a.per > a.nunits) a.per = a.nunits;
        a.nb = (a.nunits + a.per - 1) / a.per;
        a.per = (a.nunits + a.nb - 1) / a.nb;  // the bundles of equal size but the last
        a.off = off;
        off += (long long)msc_q_cols(h) * a.D;
        const size_t lds = (size_t)kC4AccWords * 4 + (size_t)a.per * unit_words * 8;
        if (lds > q->lds) q->lds = lds;
    }
    q->c4_len = (size_t)off;
    hipError_t e = hipSuccess;
    if (q->naxes) {
        e = hipMalloc((void**)&q->d_c4, q->c4_len * sizeof(int32_t));
        if (e == hipSuccess && q->lds > 64 * 1024)
            e = tsu_func_allow_lds(ctx, h->A == 2 ? reinterpret_cast<const void*>(k9_c4<2>) : reinterpret_cast<const void*>(k9_c4<1>),
                                   (int)q->lds);
    }
    if (e == hipSuccess) e = hipMalloc((void**)&q->d_tt, msc_q_tt_len(h) * sizeof(int32_t));
    if (e != hipSuccess) {
        if (q->d_c4) (void)hipFree(q->d_c4);
        if (q->d_tt) (void)hipFree(q->d_tt);
        delete q;
        return tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    h->qn = q;
    return TSU_OK;
}

// what tsu_msc_c4 and tsu_msc_quench_run ask of the lattice
int msc_c4_check(tsu_msc* h, const char* who) {
    tsu_ctx* ctx = h->ctx;
    const int len[3] = {h->g.depth, h->g.rows, h->g.cols};
    const int per[3] = {h->g.pz, h->g.pr, h->g.pc};
    TSU_REQUIRE(ctx, per[0] + per[1] + per[2] > 0, "%s: the lattice has no periodic axis (no correlator is defined)", who);
    for (int d = 0; d < 3; ++d)
        if (per[d] && len[d] > TSU_MSC_C4_MAX_AXIS)
            return tsu_fail(ctx, TSU_E_UNSUPPORTED, "%s: a periodic axis of %d sites exceeds %d (a line has to fit the LDS)", who, len[d],
                            TSU_MSC_C4_MAX_AXIS);
    return TSU_OK;
}

// the row zeroed and one launch of k9_c4 adding the counts into it (c4_len entries)
hipError_t msc_enqueue_c4(tsu_msc* h, int32_t* row, bool zero) {
    const msc_quench* q = h->qn;
    if (zero) {
        const hipError_t e = hipMemsetAsync(row, 0, q->c4_len * sizeof(int32_t), h->ctx->stream);
        if (e != hipSuccess) return e;
    }
    MscC4 p = q->plan;
    p.out = row;
    int nb = 0;
    for (int k = 0; k < q->naxes; ++k) nb = p.ax[k].nb > nb ? p.ax[k].nb : nb;
    const dim3 grid((unsigned)nb, (unsigned)(h->nT * h->W), (unsigned)q->naxes);
    if (h->A == 2) k9_c4<2><<<grid, kC4Lanes, q->lds, h->ctx->stream>>>(p);
    else k9_c4<1><<<grid, kC4Lanes, q->lds, h->ctx->stream>>>(p);
    return hipGetLastError();
}

// one launch of k9_twotime adding the counts of the planes against slot `slot` into row (msc_q_tt_len entries, zeroed by the caller)
hipError_t msc_enqueue_twotime(tsu_msc* h, int slot, int32_t* row) {
    MscTT p = {};
    p.now = h->d_s;
    p.snap = h->qn->d_snap + (size_t)slot * msc_q_plane_words(h);
    p.out = row;
    p.nsites = h->g.nsites;
    const dim3 grid((unsigned)((h->g.nsites + 256 * kTTSites - 1) / (256 * kTTSites)), (unsigned)msc_planes(h), 1);
    k9_twotime<<<grid, 256, 0, h->ctx->stream>>>(p);
    return hipGetLastError();
}

hipError_t msc_enqueue_snapshot(tsu_msc* h, int slot) {
    const size_t words = msc_q_plane_words(h);
    return hipMemcpyAsync(h->qn->d_snap + (size_t)slot * words, h->d_s, words * 8, hipMemcpyDeviceToDevice, h->ctx->stream);
}

// C4 counts of one row -> the ABI's int64 arrays, row k of each
void msc_c4_convert(const tsu_msc* h, const int32_t* host, int64_t* const out[3], size_t k) {
    const msc_quench* q = h->qn;
    const long long N = h->g.nsites;
    for (int d = 0; d < 3; ++d) {
        if (q->axis_of[d] < 0) continue;
        const MscC4Axis& a = q->plan.ax[q->axis_of[d]];
        const size_t n = msc_q_cols(h) * a.D;
        for (size_t i = 0; i < n; ++i) out[d][k * n + i] = N - 2 * (int64_t)host[a.off + i];
    }
}

int msc_c4_pointers(tsu_msc* h, const char* who, int64_t* const out[3]) {
    const int per[3] = {h->g.pz, h->g.pr, h->g.pc};
    for (int d = 0; d < 3; ++d) {
        TSU_REQUIRE(h->ctx, !per[d] || out[d], "%s: NULL output of periodic axis %d", who, d);
        TSU_REQUIRE(h->ctx, per[d] || !out[d], "%s: axis %d is open: its output must be NULL", who, d);
    }
    return TSU_OK;
}

template <typename T>
int msc_q_reserve(tsu_ctx* ctx, T*& buf, size_t& cap, size_t bytes) {
    if (cap >= bytes) return TSU_OK;
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (buf) (void)hipFree(buf);
    buf = nullptr;
    cap = 0;
    TSU_HIP_TRY(ctx, hipMalloc((void**)&buf, bytes));
    cap = bytes;
    return TSU_OK;
}

}  // namespace

void msc_quench_free(tsu_msc* h) {
    msc_quench* q = h->qn;
    if (!q) return;
    void* bufs[] = {q->d_c4, q->d_tt, q->d_snap, q->d_meas, q->d_c4h, q->d_tth};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    delete q;
    h->qn = nullptr;
}

extern "C" {

int tsu_msc_c4(tsu_msc* h, int64_t* c_z, int64_t* c_r, int64_t* c_c) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    int64_t* const out[3] = {c_z, c_r, c_c};
    int rc = msc_c4_check(h, "msc_c4");
    if (rc == TSU_OK) rc = msc_c4_pointers(h, "msc_c4", out);
    if (rc == TSU_OK) rc = msc_quench_state(h, "msc_c4");
    if (rc != TSU_OK) return rc;
    msc_quench* q = h->qn;
    TSU_HIP_TRY(ctx, msc_enqueue_c4(h, q->d_c4, true));
    std::vector<int32_t> host(q->c4_len);
    TSU_HIP_TRY(ctx, hipMemcpyAsync(host.data(), q->d_c4, host.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    msc_c4_convert(h, host.data(), out, 0);
    return TSU_OK;
}

int tsu_msc_snapshot_slots(tsu_msc* h, int n) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    TSU_REQUIRE(ctx, n >= 0 && n <= TSU_MSC_SNAPSHOT_SLOTS, "msc_snapshot_slots: n must be 0 .. %d, got %d", TSU_MSC_SNAPSHOT_SLOTS, n);
    if (!h->qn && n == 0) return TSU_OK;
    const int rc = msc_quench_state(h, "msc_snapshot_slots");
    if (rc != TSU_OK) return rc;
    msc_quench* q = h->qn;
    if (n == q->n_slots) return TSU_OK;
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // a copy or a launch in flight may still use the old slots
    const size_t words = msc_q_plane_words(h);
    uint64_t* fresh = nullptr;
    if (n > 0) {
        TSU_HIP_TRY(ctx, hipMalloc((void**)&fresh, (size_t)n * words * 8));
        const int keep = n < q->n_slots ? n : q->n_slots;
        if (keep > 0) {
            const hipError_t e = hipMemcpy(fresh, q->d_snap, (size_t)keep * words * 8, hipMemcpyDeviceToDevice);
            if (e != hipSuccess) {
                (void)hipFree(fresh);
                TSU_HIP_TRY(ctx, e);
            }
        }
    }
    if (q->d_snap) (void)hipFree(q->d_snap);
    q->d_snap = fresh;
    q->n_slots = n;
    q->taken &= (1u << n) - 1u;
    return TSU_OK;
}

int tsu_msc_snapshot(tsu_msc* h, int slot) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    TSU_REQUIRE(ctx, h->qn && slot >= 0 && slot < h->qn->n_slots, "msc_snapshot: slot %d outside the %d slots of tsu_msc_snapshot_slots",
                slot, h->qn ? h->qn->n_slots : 0);
    TSU_HIP_TRY(ctx, msc_enqueue_snapshot(h, slot));
    h->qn->taken |= 1u << slot;
    return TSU_OK;
}

int tsu_msc_snapshot_overlap(tsu_msc* h, int slot, int64_t* c) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    TSU_REQUIRE(ctx, c, "msc_snapshot_overlap: NULL output");
    TSU_REQUIRE(ctx, h->qn && slot >= 0 && slot < h->qn->n_slots && ((h->qn->taken >> slot) & 1u),
                "msc_snapshot_overlap: slot %d holds no snapshot", slot);
    msc_quench* q = h->qn;
    const size_t n = msc_q_tt_len(h);
    TSU_HIP_TRY(ctx, hipMemsetAsync(q->d_tt, 0, n * sizeof(int32_t), ctx->stream));
    TSU_HIP_TRY(ctx, msc_enqueue_twotime(h, slot, q->d_tt));
    std::vector<int32_t> host(n);
    TSU_HIP_TRY(ctx, hipMemcpyAsync(host.data(), q->d_tt, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const long long N = h->g.nsites;
    for (size_t i = 0; i < n; ++i) c[i] = N - 2 * (int64_t)host[i];
    return TSU_OK;
}

int tsu_msc_quench_run(tsu_msc* h, int n_times, const int* times, uint32_t sweep0, int n_wait, const int* wait_index) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    TSU_REQUIRE(ctx, h->have_T && h->have_seeds, "msc_quench_run: call tsu_msc_set_temperatures and tsu_msc_set_seeds first");
    TSU_REQUIRE(ctx, n_times >= 1 && times, "msc_quench_run: at least one time is needed");
    TSU_REQUIRE(ctx, times[0] >= 0, "msc_quench_run: times[0] must be >= 0");
    for (int k = 1; k < n_times; ++k) TSU_REQUIRE(ctx, times[k] > times[k - 1], "msc_quench_run: times must be strictly ascending");
    TSU_REQUIRE(ctx, (uint64_t)sweep0 + (uint64_t)times[n_times - 1] <= (1ull << 31), "msc_quench_run: sweep counter overflow");
    TSU_REQUIRE(ctx, n_wait >= 0 && n_wait <= TSU_MSC_SNAPSHOT_SLOTS && (n_wait == 0 || wait_index),
                "msc_quench_run: n_wait must be 0 .. %d", TSU_MSC_SNAPSHOT_SLOTS);
    for (int j = 0; j < n_wait; ++j)
        TSU_REQUIRE(ctx, wait_index[j] >= 0 && wait_index[j] < n_times && (j == 0 || wait_index[j] > wait_index[j - 1]),
                    "msc_quench_run: wait_index must be strictly ascending indices into times");
    int rc = msc_c4_check(h, "msc_quench_run");
    if (rc == TSU_OK) rc = msc_quench_state(h, "msc_quench_run");
    if (rc != TSU_OK) return rc;
    msc_quench* q = h->qn;
    TSU_REQUIRE(ctx, n_wait <= q->n_slots, "msc_quench_run: %d waiting times need tsu_msc_snapshot_slots(h, n >= %d) first (%d slots)", n_wait,
                n_wait, q->n_slots);
    q->n_times = 0;
    const size_t row_len = msc_row_len(h), tt_len = msc_q_tt_len(h);
    const size_t mbytes = (size_t)n_times * row_len * 8, cbytes = (size_t)n_times * q->c4_len * sizeof(int32_t);
    const size_t tbytes = (size_t)n_wait * n_times * tt_len * sizeof(int32_t);
    rc = msc_q_reserve(ctx, q->d_meas, q->meas_cap, mbytes);
    if (rc == TSU_OK) rc = msc_q_reserve(ctx, q->d_c4h, q->c4h_cap, cbytes);
    if (rc == TSU_OK && tbytes) rc = msc_q_reserve(ctx, q->d_tth, q->tth_cap, tbytes);
    if (rc != TSU_OK) return rc;
    TSU_HIP_TRY(ctx, hipMemsetAsync(q->d_meas, 0, mbytes, ctx->stream));
    TSU_HIP_TRY(ctx, hipMemsetAsync(q->d_c4h, 0, cbytes, ctx->stream));
    if (tbytes) TSU_HIP_TRY(ctx, hipMemsetAsync(q->d_tth, 0, tbytes, ctx->stream));
    unsigned long long spans = 0;  // the small route starts a launch per span; the handle counts tsu_msc_sweep's
    int done = 0, waits = 0;
    for (int k = 0; k < n_times; ++k) {
        TSU_HIP_TRY(ctx, msc_enqueue_sweeps(h, times[k] - done, sweep0 + (uint32_t)done, &spans));
        done = times[k];
        TSU_HIP_TRY(ctx, msc_enqueue_measure(h, q->d_meas + (size_t)k * row_len));
        TSU_HIP_TRY(ctx, msc_enqueue_c4(h, q->d_c4h + (size_t)k * q->c4_len, false));
        if (waits < n_wait && wait_index[waits] == k) {
            TSU_HIP_TRY(ctx, msc_enqueue_snapshot(h, waits));
            q->taken |= 1u << waits;
            ++waits;
        }
        for (int j = 0; j < waits; ++j) TSU_HIP_TRY(ctx, msc_enqueue_twotime(h, j, q->d_tth + ((size_t)j * n_times + k) * tt_len));
    }
    h->launches += h->route == TSU_MSC_ROUTE_SMALL ? (done > 0 ? 1 : 0) : spans;
    q->n_times = n_times;
    q->n_wait = n_wait;
    for (int j = 0; j < n_wait; ++j) q->wait_index[j] = wait_index[j];
    return TSU_OK;
}

int tsu_msc_quench_history(tsu_msc* h, int n_times, int64_t* unsat, int64_t* sum, int64_t* q_out, int64_t* q_link, int64_t* c_z,
                           int64_t* c_r, int64_t* c_c, int64_t* two_time) {
    TSU_ENTER(h ? h->ctx : nullptr);
    if (!h) return TSU_E_INVALID;
    tsu_ctx* ctx = h->ctx;
    msc_quench* q = h->qn;
    TSU_REQUIRE(ctx, q && q->n_times > 0, "msc_quench_history: no quench run has been recorded");
    TSU_REQUIRE(ctx, n_times == q->n_times, "msc_quench_history: the last run recorded %d times, not %d", q->n_times, n_times);
    TSU_REQUIRE(ctx, unsat && sum, "msc_quench_history: NULL output");
    TSU_REQUIRE(ctx, two_time || q->n_wait == 0, "msc_quench_history: NULL two_time with %d waiting times", q->n_wait);
    int64_t* const out[3] = {c_z, c_r, c_c};
    const int rc = msc_c4_pointers(h, "msc_quench_history", out);
    if (rc != TSU_OK) return rc;
    const size_t row_len = msc_row_len(h), tt_len = msc_q_tt_len(h), nt = (size_t)n_times;
    std::vector<unsigned long long> meas(nt * row_len);
    std::vector<int32_t> c4(nt * q->c4_len), tt((size_t)q->n_wait * nt * tt_len);
    TSU_HIP_TRY(ctx, hipMemcpyAsync(meas.data(), q->d_meas, meas.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipMemcpyAsync(c4.data(), q->d_c4h, c4.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (!tt.empty()) TSU_HIP_TRY(ctx, hipMemcpyAsync(tt.data(), q->d_tth, tt.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const size_t col = (size_t)h->W * 64, n1 = (size_t)h->nT * h->A * col, nq = (size_t)h->nT * col;
    const long long N = h->g.nsites, nb = msc_bonds(h->g);
    for (size_t k = 0; k < nt; ++k) {
        const unsigned long long* row = meas.data() + k * row_len;
        for (size_t i = 0; i < n1; ++i) {
            unsat[k * n1 + i] = (int64_t)row[i];
            sum[k * n1 + i] = 2 * (int64_t)row[n1 + i] - N;
        }
        if (h->A == 2)
            for (size_t i = 0; i < nq; ++i) {
                if (q_out) q_out[k * nq + i] = N - 2 * (int64_t)row[2 * n1 + i];
                if (q_link) q_link[k * nq + i] = nb - 2 * (int64_t)row[2 * n1 + nq + i];
            }
        msc_c4_convert(h, c4.data() + k * q->c4_len, out, k);
    }
    for (int j = 0; j < q->n_wait; ++j)
        for (size_t k = 0; k < nt; ++k)
            for (size_t i = 0; i < tt_len; ++i) {
                const size_t at = ((size_t)j * nt + k) * tt_len + i;
                two_time[at] = (int)k < q->wait_index[j] ? 0 : N - 2 * (int64_t)tt[at];
            }
    return TSU_OK;
}

}  // extern "C"

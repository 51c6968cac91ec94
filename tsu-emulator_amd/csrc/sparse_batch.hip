// sparse_batch.hip -- K5 walker batches: n_ladders ladders of n_temps walkers on the CSR graph of one tsu_sparse handle (gfx950).
//
// No reference counterpart: the reference tempers a dense matrix replica by replica on the host (gibbs.py:238-338) and anneals one
// state at a time.  Here the half-sweeps, the energies and the swap passes of all walkers are batched launches and a run waits for
// nothing (contract: DESIGN.md section 3, "Walker batches on a sparse graph"; kernels and routes: sparse_batch_dev.h, section 5).
// The handle is a lean struct of its own: the lattice ladders' pt_ladder / pt_host.h carry spin planes, disorder and correlation
// state that a graph does not have; what is shared is the swap pass k7_pt_swap (pt_dev.h), enqueued by the ladders' own
// pt_enqueue_swap (pt_host.h); nothing else of pt_host.h is used here.
#include <cmath>
#include <limits>
#include <new>
#include <vector>

#include "pt_host.h"  // pt_enqueue_swap: the one launch of the swap pass
#include "sparse.h"
#include "sparse_batch_dev.h"

struct tsu_sparse_batch {
    tsu_ctx* ctx;
    tsu_sparse* g;      // borrowed
    int R, nl, nw, WP;  // temperatures, ladders, walkers, padded walkers (bytes per position)
    int nseg;           // energy segments
    int have_T, have_init;
    uint32_t sweeps, rounds;
    unsigned long long launches;  // kernel launches enqueued by run
    int hist_rounds;
    size_t hist_cap;
    uint32_t key0, key1;
    int8_t* d_state;    // [n][WP]
    int8_t* d_stage;    // n bytes, site order
    int32_t* d_slot;    // [ladder][walker] -> slot
    int32_t* d_was;     // [ladder][slot] -> walker
    int32_t* d_flag;
    double* d_T;        // slot -> T
    long long* d_att;   // [ladder][pair]
    long long* d_acc;
    long long* d_trips;
    double* d_part;     // [segment][WP]
    long long* d_mpart;
    double* d_E;        // walker -> E of the last energy pass
    long long* d_M;
    double* d_hE;       // [round][ladder][slot]
    long long* d_hM;
    int32_t* d_hW;
    // best states (track_best)
    int track, best_pending;  // best_pending: the current states have not been candidates yet
    int8_t* d_best;     // [n][WP]
    double* d_bestE;    // walker -> lowest energy so far (+inf: none)
};

namespace {

void k5b_free_history(tsu_sparse_batch* b) {
    void* bufs[] = {b->d_hE, b->d_hM, b->d_hW};
    for (void* p : bufs)
        if (p) (void)hipFree(p);
    b->d_hE = nullptr;
    b->d_hM = nullptr;
    b->d_hW = nullptr;
    b->hist_cap = 0;
}

void k5b_free(tsu_sparse_batch* b) {
    void* bufs[] = {b->d_state, b->d_stage, b->d_slot, b->d_was, b->d_flag, b->d_T, b->d_att, b->d_acc, b->d_trips,
                    b->d_part, b->d_mpart, b->d_E, b->d_M, b->d_best, b->d_bestE};
    for (void* p : bufs)
        if (p) (void)hipFree(p);
    k5b_free_history(b);
    delete b;
}

K5BArgs k5b_args(const tsu_sparse_batch* b) {
    K5BArgs A;
    A.row_ptr = b->g->row_ptr;
    A.col = b->g->col;
    A.val = b->g->val;
    A.bias = b->g->bias;
    A.site_of = b->g->site_of;
    A.state = b->d_state;
    A.slot = b->d_slot;
    A.T = b->d_T;
    A.n = b->g->n;
    A.nw = b->nw;
    A.WP = b->WP;
    A.k0 = b->key0;
    A.k1 = b->key1;
    return A;
}

// the small route: graphs k5_small takes, unless TSU_K5B_SMALL=0 (read per call)
bool k5b_small_route(const tsu_sparse_batch* b) { return b->g->n <= K5S_MAX && k5_env_on("TSU_K5B_SMALL"); }

// Walkers per thread of the colour route: 4 up to 4 walkers, 8 beyond.  Measured at 2^20 sites, mean degree 6, 32 walkers: 4 and 8
// per thread tie (1.16e11 walker-updates/s), 16 per thread is 12 % slower (74 registers, 6 waves per SIMD); 8 reads the CSR row half
// as often as 4 (profiles/sparse_batch_time.txt).  TSU_K5B_CHUNK=4|8|16 (read per call) forces one.
int k5b_chunk(const tsu_sparse_batch* b) {
    if (const char* e = getenv("TSU_K5B_CHUNK")) {
        const int w = atoi(e);
        if (w == 4 || w == 8 || w == 16) return w;
    }
    return b->nw <= 4 ? 4 : 8;
}

unsigned k5b_blocks(long long threads) { return (unsigned)((threads + 255) / 256); }

template <int W>
void k5b_launch_color(const tsu_sparse_batch* b, const K5BArgs& A, int pb, int pe, uint32_t sweep) {
    const long long threads = (long long)(pe - pb) * ((b->nw + W - 1) / W);
    k5b_color<W><<<k5b_blocks(threads), 256, 0, b->ctx->stream>>>(A, pb, pe, sweep);
}

// every walker's E and sum of spins into d_E / d_M by the colour route's passes (two launches; asynchronous)
void k5b_enqueue_energies(tsu_sparse_batch* b) {
    const K5BArgs A = k5b_args(b);
    // (at most 8 walkers per thread here: 16 running sums beside 16 fields do not fit the 128 registers of a 1024-thread workgroup)
    const int W = k5b_chunk(b) == 4 ? 4 : 8;
    const dim3 grid((unsigned)b->nseg, (unsigned)((b->nw + W - 1) / W));
    hipStream_t st = b->ctx->stream;
    if (W == 4) k5b_energy<4><<<grid, K5B_THREADS, 0, st>>>(A, b->d_part, b->d_mpart);
    else k5b_energy<8><<<grid, K5B_THREADS, 0, st>>>(A, b->d_part, b->d_mpart);
    k5b_energy_final<<<k5b_blocks(b->nw), 256, 0, st>>>(b->d_part, b->d_mpart, b->nseg, b->nw, b->WP, b->d_E, b->d_M);
}

// the states as they stand become candidates for the best states (d_E holds their energies): copy, then min update
void k5b_enqueue_best(tsu_sparse_batch* b) {
    hipStream_t st = b->ctx->stream;
    k5b_best_copy<<<k5b_blocks((long long)b->g->n * (b->WP / 4)), 256, 0, st>>>(b->d_state, b->d_best, b->d_E, b->d_bestE, b->g->n, b->nw, b->WP);
    k5b_best_min<<<k5b_blocks(b->nw), 256, 0, st>>>(b->d_E, b->d_bestE, b->nw);
}

// g = the walker now at (ladder, slot); `op` names the entry point (synchronises)
int k5b_at(tsu_sparse_batch* b, int ladder, int slot, const char* op, int* g) {
    tsu_ctx* ctx = b->ctx;
    TSU_REQUIRE(ctx, ladder >= 0 && ladder < b->nl && slot >= 0 && slot < b->R,
                "tsu_sparse_batch_%s: ladder %d, slot %d out of range (%d ladder(s) of %d temperatures)", op, ladder, slot, b->nl, b->R);
    int32_t w = -1;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(&w, b->d_was + (size_t)ladder * b->R + slot, sizeof(w), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (w < 0 || w >= b->R) return tsu_fail(ctx, TSU_E_HIP, "tsu_sparse_batch_%s: corrupt slot table (walker %d)", op, (int)w);
    *g = ladder * b->R + w;
    return TSU_OK;
}

}  // namespace

extern "C" {

int tsu_sparse_batch_create(tsu_sparse* graph, int n_temps, int n_ladders, tsu_sparse_batch** out) {
    TSU_ENTER(graph ? graph->ctx : nullptr);
    if (!graph) return TSU_E_INVALID;
    tsu_ctx* ctx = graph->ctx;
    TSU_REQUIRE(ctx, out, "tsu_sparse_batch_create: NULL output");
    *out = nullptr;
    TSU_REQUIRE(ctx, n_temps >= 1 && n_temps <= kPtMaxTemps, "tsu_sparse_batch_create: n_temps must be in [1, %d], got %d", kPtMaxTemps, n_temps);
    TSU_REQUIRE(ctx, n_ladders >= 1, "tsu_sparse_batch_create: n_ladders must be >= 1, got %d", n_ladders);
    TSU_REQUIRE(ctx, (long long)n_temps * n_ladders <= 65535, "tsu_sparse_batch_create: at most 65535 walkers, got %d x %d", n_ladders, n_temps);
    const int nw = n_temps * n_ladders, WP = (nw + K5B_PAD - 1) / K5B_PAD * K5B_PAD;
    TSU_REQUIRE(ctx, graph->n < (1 << 30) && (long long)graph->n * WP < (1ll << 38), "tsu_sparse_batch_create: %d sites x %d walkers is too large",
                graph->n, nw);
    tsu_sparse_batch* b = new (std::nothrow) tsu_sparse_batch();
    if (!b) return tsu_fail(ctx, TSU_E_NOMEM, "tsu_sparse_batch_create: host allocation failed");
    b->ctx = ctx;
    b->g = graph;
    b->R = n_temps;
    b->nl = n_ladders;
    b->nw = nw;
    b->WP = WP;
    b->nseg = (graph->n + K5B_SEGMENT - 1) / K5B_SEGMENT;
    const size_t n = (size_t)graph->n, pairs = (size_t)n_ladders * (n_temps - 1);
    hipError_t e = hipSuccess;
    auto alloc = [&e](auto*& ptr, size_t bytes) {
        if (e == hipSuccess) e = hipMalloc((void**)&ptr, bytes ? bytes : 8);
    };
    alloc(b->d_state, n * WP);
    alloc(b->d_stage, n);
    alloc(b->d_slot, nw * sizeof(int32_t));
    alloc(b->d_was, nw * sizeof(int32_t));
    alloc(b->d_flag, nw * sizeof(int32_t));
    alloc(b->d_T, n_temps * sizeof(double));
    alloc(b->d_att, pairs * sizeof(long long));
    alloc(b->d_acc, pairs * sizeof(long long));
    alloc(b->d_trips, nw * sizeof(long long));
    alloc(b->d_part, (size_t)b->nseg * WP * sizeof(double));
    alloc(b->d_mpart, (size_t)b->nseg * WP * sizeof(long long));
    alloc(b->d_E, nw * sizeof(double));
    alloc(b->d_M, nw * sizeof(long long));
    if (e == hipSuccess) e = hipMemsetAsync(b->d_state, 0, n * WP, ctx->stream);
    if (e == hipSuccess) {
        k5b_reset<<<k5b_blocks(nw), 256, 0, ctx->stream>>>(b->d_slot, b->d_was, b->d_flag, b->d_att, b->d_acc, b->d_trips, n_temps, nw);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        k5b_free(b);
        (void)hipGetLastError();
        return tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "tsu_sparse_batch_create: %s", hipGetErrorString(e));
    }
    *out = b;
    return TSU_OK;
}

int tsu_sparse_batch_destroy(tsu_sparse_batch* b) {
    TSU_ENTER(b ? b->ctx : nullptr);
    if (!b) return TSU_OK;
    (void)hipStreamSynchronize(b->ctx->stream);
    k5b_free(b);
    return TSU_OK;
}

int tsu_sparse_batch_set_temperatures(tsu_sparse_batch* b, const double* T) {
    TSU_ENTER(b ? b->ctx : nullptr);
    if (!b) return TSU_E_INVALID;
    tsu_ctx* ctx = b->ctx;
    TSU_REQUIRE(ctx, T, "tsu_sparse_batch_set_temperatures: NULL temperatures");
    K5BTemps t;
    for (int i = 0; i < kPtMaxTemps; ++i) t.T[i] = 1.0;
    for (int i = 0; i < b->R; ++i) {
        TSU_REQUIRE(ctx, T[i] > 0.0 && std::isfinite(T[i]), "Temperature must be positive (tsu_sparse_batch_set_temperatures: T[%d] = %g)", i, T[i]);
        t.T[i] = T[i];
    }
    k5b_set_temps<<<1, 256, 0, ctx->stream>>>(t, b->R, b->d_T);
    TSU_HIP_TRY(ctx, hipGetLastError());
    b->have_T = 1;
    return TSU_OK;
}

int tsu_sparse_batch_init(tsu_sparse_batch* b, uint64_t seed, int initial) {
    TSU_ENTER(b ? b->ctx : nullptr);
    if (!b) return TSU_E_INVALID;
    tsu_ctx* ctx = b->ctx;
    TSU_REQUIRE(ctx, initial == 0 || initial == 1 || initial == -1, "tsu_sparse_batch_init: initial must be 0 (random), 1 (ones) or -1 (zeros), got %d",
                initial);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    hipStream_t st = ctx->stream;
    k5b_init<<<k5b_blocks((long long)b->g->n * (b->WP / 4)), 256, 0, st>>>(b->d_state, b->g->site_of, b->g->n, b->nw, b->WP, initial, k0, k1);
    k5b_reset<<<k5b_blocks(b->nw), 256, 0, st>>>(b->d_slot, b->d_was, b->d_flag, b->d_att, b->d_acc, b->d_trips, b->R, b->nw);
    if (b->d_bestE) k5b_fill<<<k5b_blocks(b->nw), 256, 0, st>>>(b->d_bestE, std::numeric_limits<double>::infinity(), b->nw);
    TSU_HIP_TRY(ctx, hipGetLastError());
    TSU_HIP_TRY(ctx, hipStreamSynchronize(st));
    b->key0 = k0;
    b->key1 = k1;
    b->sweeps = b->rounds = 0;
    b->hist_rounds = 0;
    b->best_pending = 1;
    b->have_init = 1;
    return TSU_OK;
}

int tsu_sparse_batch_set_state(tsu_sparse_batch* b, int ladder, int slot, const int8_t* bits_host) {
    TSU_ENTER(b ? b->ctx : nullptr);
    if (!b) return TSU_E_INVALID;
    tsu_ctx* ctx = b->ctx;
    const int n = b->g->n;
    TSU_REQUIRE(ctx, bits_host, "tsu_sparse_batch_set_state: NULL buffer");
    for (int i = 0; i < n; ++i) TSU_REQUIRE(ctx, bits_host[i] == 0 || bits_host[i] == 1, "tsu_sparse_batch_set_state: state must be 0/1");
    int g = 0;
    const int rc = k5b_at(b, ladder, slot, "set_state", &g);
    if (rc != TSU_OK) return rc;
    TSU_HIP_TRY(ctx, hipMemcpyAsync(b->d_stage, bits_host, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    k5b_scatter<<<k5b_blocks(n), 256, 0, ctx->stream>>>(b->d_stage, b->g->site_of, b->d_state, n, b->WP, g);
    TSU_HIP_TRY(ctx, hipGetLastError());
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    b->best_pending = 1;
    return TSU_OK;
}

int tsu_sparse_batch_get_state(tsu_sparse_batch* b, int ladder, int slot, int8_t* bits_host) {
    TSU_ENTER(b ? b->ctx : nullptr);
    if (!b) return TSU_E_INVALID;
    tsu_ctx* ctx = b->ctx;
    const int n = b->g->n;
    TSU_REQUIRE(ctx, bits_host, "tsu_sparse_batch_get_state: NULL buffer");
    int g = 0;
    const int rc = k5b_at(b, ladder, slot, "get_state", &g);
    if (rc != TSU_OK) return rc;
    k5b_gather<<<k5b_blocks(n), 256, 0, ctx->stream>>>(b->d_state, b->g->site_of, b->d_stage, n, b->WP, g);
    TSU_HIP_TRY(ctx, hipGetLastError());
    TSU_HIP_TRY(ctx, hipMemcpyAsync(bits_host, b->d_stage, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int tsu_sparse_batch_run(tsu_sparse_batch* b, int n_rounds, int swap_interval, int do_swap, int record) {
    TSU_ENTER(b ? b->ctx : nullptr);
    if (!b) return TSU_E_INVALID;
    tsu_ctx* ctx = b->ctx;
    tsu_sparse* g = b->g;
    TSU_REQUIRE(ctx, b->have_T, "tsu_sparse_batch_run: call tsu_sparse_batch_set_temperatures first");
    TSU_REQUIRE(ctx, b->have_init, "tsu_sparse_batch_run: call tsu_sparse_batch_init first");
    TSU_REQUIRE(ctx, n_rounds >= 0 && swap_interval >= 1, "tsu_sparse_batch_run: need n_rounds >= 0 and swap_interval >= 1 (got %d, %d)", n_rounds,
                swap_interval);
    TSU_REQUIRE(ctx, (uint64_t)b->sweeps + (uint64_t)n_rounds * (uint64_t)swap_interval <= (1ull << 31), "tsu_sparse_batch_run: sweep counter overflow");
    TSU_REQUIRE(ctx, (uint64_t)b->rounds + (uint64_t)n_rounds <= 0xFFFFFFFFull, "tsu_sparse_batch_run: round counter overflow");
    const int R = b->R, nl = b->nl;
    if (record && b->hist_cap < (size_t)n_rounds) {
        TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // no kernel still writes the rows
        k5b_free_history(b);
        const size_t rows = (size_t)n_rounds * b->nw;
        hipError_t e = hipMalloc((void**)&b->d_hE, rows * sizeof(double));
        if (e == hipSuccess) e = hipMalloc((void**)&b->d_hM, rows * sizeof(long long));
        if (e == hipSuccess) e = hipMalloc((void**)&b->d_hW, rows * sizeof(int32_t));
        if (e != hipSuccess) {
            k5b_free_history(b);
            b->hist_rounds = 0;
            (void)hipGetLastError();
            return tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "tsu_sparse_batch_run: history of %d rounds: %s", n_rounds,
                            hipGetErrorString(e));
        }
        b->hist_cap = (size_t)n_rounds;
    }
    b->hist_rounds = record ? n_rounds : 0;
    const bool small = k5b_small_route(b);
    const int W = k5b_chunk(b);
    const K5BArgs A = k5b_args(b);
    const int* d_off = (const int*)(g->site_of + g->n);  // the colour offsets sit behind the site table (tsu_sparse_create)
    hipStream_t st = ctx->stream;
    if (b->track && b->best_pending && n_rounds > 0) {  // the states the run starts from are candidates
        k5b_enqueue_energies(b);
        k5b_enqueue_best(b);
        b->launches += 4;
        b->best_pending = 0;
    }
    PTSwap sw;
    sw.E = b->d_E;
    sw.M = b->d_M;
    sw.T = b->d_T;
    sw.was = b->d_was;
    sw.slot = b->d_slot;
    sw.flag = b->d_flag;
    sw.att = b->d_att;
    sw.acc = b->d_acc;
    sw.trips = b->d_trips;
    sw.R = R;
    sw.do_swap = do_swap ? 1 : 0;
    sw.k0 = b->key0;
    sw.k1 = b->key1;
    sw.nl = nl;
    sw.skey = nullptr;
    const bool need_E = do_swap || record || b->track;
    for (int t = 0; t < n_rounds; ++t) {
        if (small) {  // the round's sweeps and the energies in one launch
            k5b_small<<<(unsigned)b->nw, K5B_THREADS, (size_t)((g->n + 15) / 16 * 16), st>>>(A, d_off, g->n_colors, swap_interval, b->sweeps, b->d_E,
                                                                                            b->d_M);
            b->launches += 1;
        } else {
            for (int s = 0; s < swap_interval; ++s)
                for (int c = 0; c < g->n_colors; ++c) {
                    const int pb = g->color_off[c], pe = g->color_off[c + 1];
                    if (pe <= pb) continue;
                    if (W == 4) k5b_launch_color<4>(b, A, pb, pe, b->sweeps + (uint32_t)s);
                    else if (W == 8) k5b_launch_color<8>(b, A, pb, pe, b->sweeps + (uint32_t)s);
                    else k5b_launch_color<16>(b, A, pb, pe, b->sweeps + (uint32_t)s);
                    b->launches += 1;
                }
            if (need_E) {
                k5b_enqueue_energies(b);
                b->launches += 2;
            }
        }
        b->sweeps += (uint32_t)swap_interval;
        if (b->track) {
            k5b_enqueue_best(b);
            b->launches += 2;
        }
        if (do_swap || record) {
            const size_t row = (size_t)t * b->nw;
            sw.hE = record ? b->d_hE + row : nullptr;
            sw.hM = record ? b->d_hM + row : nullptr;
            sw.hW = record ? b->d_hW + row : nullptr;
            sw.t = b->rounds;
            pt_enqueue_swap(sw, (unsigned)nl, st);
            b->launches += 1;
        }
        b->rounds += 1;
    }
    TSU_HIP_TRY(ctx, hipGetLastError());
    return TSU_OK;
}

int tsu_sparse_batch_history(tsu_sparse_batch* b, double* E, int64_t* M, int32_t* walker) {
    TSU_ENTER(b ? b->ctx : nullptr);
    if (!b) return TSU_E_INVALID;
    tsu_ctx* ctx = b->ctx;
    const size_t n = (size_t)b->hist_rounds * b->nw;
    if (n) {
        if (E) TSU_HIP_TRY(ctx, hipMemcpyAsync(E, b->d_hE, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (M) TSU_HIP_TRY(ctx, hipMemcpyAsync(M, b->d_hM, n * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        if (walker) TSU_HIP_TRY(ctx, hipMemcpyAsync(walker, b->d_hW, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int tsu_sparse_batch_stats(tsu_sparse_batch* b, int64_t* attempts, int64_t* accepts, int64_t* round_trips, int32_t* walker_at_slot,
                           uint64_t* sweep_count) {
    TSU_ENTER(b ? b->ctx : nullptr);
    if (!b) return TSU_E_INVALID;
    tsu_ctx* ctx = b->ctx;
    const size_t pairs = (size_t)b->nl * (b->R - 1), nw = (size_t)b->nw;
    if (attempts && pairs) TSU_HIP_TRY(ctx, hipMemcpyAsync(attempts, b->d_att, pairs * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (accepts && pairs) TSU_HIP_TRY(ctx, hipMemcpyAsync(accepts, b->d_acc, pairs * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (round_trips) TSU_HIP_TRY(ctx, hipMemcpyAsync(round_trips, b->d_trips, nw * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    if (walker_at_slot) TSU_HIP_TRY(ctx, hipMemcpyAsync(walker_at_slot, b->d_was, nw * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (sweep_count) *sweep_count = b->sweeps;
    return TSU_OK;
}

int tsu_sparse_batch_energies(tsu_sparse_batch* b, double* E, int64_t* sum_s) {
    TSU_ENTER(b ? b->ctx : nullptr);
    if (!b) return TSU_E_INVALID;
    tsu_ctx* ctx = b->ctx;
    k5b_enqueue_energies(b);
    TSU_HIP_TRY(ctx, hipGetLastError());
    if (E) TSU_HIP_TRY(ctx, hipMemcpyAsync(E, b->d_E, (size_t)b->nw * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (sum_s) TSU_HIP_TRY(ctx, hipMemcpyAsync(sum_s, b->d_M, (size_t)b->nw * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSU_OK;
}

int tsu_sparse_batch_track_best(tsu_sparse_batch* b, int enable) {
    TSU_ENTER(b ? b->ctx : nullptr);
    if (!b) return TSU_E_INVALID;
    tsu_ctx* ctx = b->ctx;
    if (!enable) {
        b->track = 0;
        return TSU_OK;
    }
    if (!b->d_best) {
        hipError_t e = hipMalloc((void**)&b->d_best, (size_t)b->g->n * b->WP);
        if (e == hipSuccess) e = hipMalloc((void**)&b->d_bestE, (size_t)b->nw * sizeof(double));
        if (e == hipSuccess) e = hipMemsetAsync(b->d_best, 0, (size_t)b->g->n * b->WP, ctx->stream);
        if (e != hipSuccess) {
            if (b->d_best) (void)hipFree(b->d_best);
            if (b->d_bestE) (void)hipFree(b->d_bestE);
            b->d_best = nullptr;
            b->d_bestE = nullptr;
            (void)hipGetLastError();
            return tsu_fail(ctx, e == hipErrorOutOfMemory ? TSU_E_NOMEM : TSU_E_HIP, "tsu_sparse_batch_track_best: %s", hipGetErrorString(e));
        }
        k5b_fill<<<k5b_blocks(b->nw), 256, 0, ctx->stream>>>(b->d_bestE, std::numeric_limits<double>::infinity(), b->nw);
        TSU_HIP_TRY(ctx, hipGetLastError());
    }
    if (!b->track) b->best_pending = 1;  // whatever ran untracked: the states as they stand are the next candidates
    b->track = 1;
    return TSU_OK;
}

int tsu_sparse_batch_best(tsu_sparse_batch* b, int ladder, double* E, int8_t* bits_host, int32_t* walker) {
    TSU_ENTER(b ? b->ctx : nullptr);
    if (!b) return TSU_E_INVALID;
    tsu_ctx* ctx = b->ctx;
    TSU_REQUIRE(ctx, ladder >= 0 && ladder < b->nl, "tsu_sparse_batch_best: ladder %d out of range (%d ladder(s))", ladder, b->nl);
    TSU_REQUIRE(ctx, b->d_bestE, "tsu_sparse_batch_best: call tsu_sparse_batch_track_best first");
    std::vector<double> be((size_t)b->R);
    TSU_HIP_TRY(ctx, hipMemcpyAsync(be.data(), b->d_bestE + (size_t)ladder * b->R, be.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    int w = 0;
    for (int i = 1; i < b->R; ++i)
        if (be[(size_t)i] < be[(size_t)w]) w = i;
    TSU_REQUIRE(ctx, std::isfinite(be[(size_t)w]), "tsu_sparse_batch_best: no tracked run yet");
    if (E) *E = be[(size_t)w];
    if (walker) *walker = w;
    if (bits_host) {
        const int n = b->g->n;
        k5b_gather<<<k5b_blocks(n), 256, 0, ctx->stream>>>(b->d_best, b->g->site_of, b->d_stage, n, b->WP, ladder * b->R + w);
        TSU_HIP_TRY(ctx, hipGetLastError());
        TSU_HIP_TRY(ctx, hipMemcpyAsync(bits_host, b->d_stage, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        TSU_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return TSU_OK;
}

int tsu_sparse_batch_plan(tsu_sparse_batch* b, int32_t* rec) {
    if (!b) return TSU_E_INVALID;
    TSU_REQUIRE(b->ctx, rec, "tsu_sparse_batch_plan: NULL output");
    const bool small = k5b_small_route(b);
    int classes = 0;
    for (int c = 0; c < b->g->n_colors; ++c) classes += b->g->color_off[c + 1] > b->g->color_off[c] ? 1 : 0;
    rec[0] = small ? 1 : 0;
    rec[1] = small ? 1 : k5b_chunk(b);
    rec[2] = b->WP;
    rec[3] = small ? 0 : classes;
    rec[4] = (small ? 1 : 2) + 1 + (b->track ? 2 : 0);
    rec[5] = b->nseg;
    return TSU_OK;
}

int tsu_sparse_batch_launch_count(tsu_sparse_batch* b, uint64_t* n_launches) {
    if (!b || !n_launches) return TSU_E_INVALID;
    *n_launches = b->launches;
    return TSU_OK;
}

}  // extern "C"

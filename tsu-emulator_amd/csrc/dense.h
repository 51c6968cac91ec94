// dense.h -- state of one dense coupling system (K2) and the device helpers its kernels share.
#pragma once
#include "tsu_common.h"
#include "dense_plan.h"

struct tsu_dense {
    tsu_ctx* ctx;
    int n, dtype;
    void* J;    // n x n row-major, f64 or f32
    void* JT;   // transpose (aliases J when J is symmetric)
    double* bias;
    int8_t* state;   // current state ({0,1})
    int8_t* state2;  // next state: a sweep reads `state` (frozen) and writes `state2`, then the two are swapped
    double* field;
    int64_t* order;  // device copy of the visiting order (n_sweeps * n) or NULL
    double* uniforms;
    size_t order_cap, uni_cap;  // bytes allocated (so are all *_cap below: dense_grow)
    double* d_energy;
    int8_t* backup;     // state at the start of a one-launch call (restored when a kernel gives up half way)
    // cooperative single-launch path (dense_coop.hip)
    double* co_logit;   // logit(u) per site for the current sweep
    double* co_corr;    // intra-superblock correction per site
    int8_t* co_d0;      // flips decided from the field alone
    int8_t* co_d1;      // current flips of the fixed-point iteration
    int* co_lists;      // two change lists of SB_SIZE entries
    int* co_counts;     // per (sweep, superblock): changes per iteration
    unsigned* co_bar;   // grid barrier counter, error flag, slowest fixed point, not-converged flag
    size_t co_counts_cap;
    int8_t* samples;    // device buffer of recorded states (tsu_dense_sample)
    size_t samples_cap;
    double* temps;      // device copy of an annealing schedule (tsu_dense_anneal)
    size_t temps_cap;
    void* rep_buf;      // tsu_dense_sweep_replicas: states, replayed uniforms and per-replica parameters
    size_t rep_cap;
    unsigned* h_flags;      // pinned host words: a one-launch kernel's error flags land here without a staged copy
    int8_t* h_rep;          // pinned host buffer of 8 n bytes: a group of replica states travels in ONE copy each way
    int8_t* h_stage;        // pinned host buffer (n bytes + 8): get_state / energy come back through it (a copy into the caller's
                            // pageable memory is staged by the runtime and costs ~10 us more)
    unsigned long long* pp_masks;  // k2_pipe: flip-mask granules of the solver teams
    double* co_fields;  // [n] fields of d->state as the last one-launch call left it (kept: when they are valid)
    DenseKept kept;     // the fields kept from call to call and the sticky switches (dense_plan.h)
    // owner-computes kernel (dense_own.hip): value-mask granules of the running generation and of the superblocks' final values
    unsigned long long* own_gran;
    size_t own_cap;
    uint64_t n_own, n_pipe;  // successful launches of k2_own / k2_pipe (tsu_dense_launch_counts)
};

// per-replica parameters of a k2_own launch
struct OwnRep {
    double T;
    uint32_t sweep0, tag, k0, k1;
    int src;  // (several replicas, fields kept) which of the previous call's replicas this state is: row of its fields
};


static __device__ __forceinline__ double dense_uniform(uint32_t i, uint32_t t, uint32_t tag, uint32_t k0, uint32_t k1) {
    u32x4 w = tsu_philox(i >> 1, 0u, t, tag, k0, k1);
    uint32_t a = (i & 1) ? w.z : w.x, b = (i & 1) ? w.w : w.y;
    a >>= 5;
    b >>= 6;
    return ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
}

static __device__ __forceinline__ double sigmoid_clamped(double x) {
    if (x > 20.0) return 1.0;
    if (x < -20.0) return 0.0;
    return 1.0 / (1.0 + exp(-x));
}


// grow-only device buffer: reallocated (contents dropped) only when it holds fewer than `bytes`; no memset, no synchronisation
template <typename T>
static inline hipError_t dense_grow(T*& p, size_t& cap, size_t bytes) {
    if (cap >= bytes) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    const hipError_t e = hipMalloc((void**)&p, bytes);
    if (e == hipSuccess) cap = bytes;
    return e;
}


// One K2 call on d->state: n_sweeps sweeps with the state recorded into samples_dev after rec_from, rec_from + rec_every, ... of them.
struct DenseCall {
    double T;
    const double* temps_dev;     // one temperature per sweep, or nullptr: T
    int n_sweeps, rec_from, rec_every;
    int8_t* samples_dev;
    uint64_t seed;
    uint32_t sweep0, replica;
    const double* uniforms_dev;  // [n_sweeps][n] replayed uniforms or nullptr
    const int64_t* order_dev;    // [n_sweeps][n] visiting orders or nullptr
    bool plain;                  // no recorded states, no schedule
};
// the Philox stream of (seed, replica): counter word 3 and the key
struct DenseStream {
    uint32_t tag, k0, k1;
};
static inline DenseStream dense_stream(uint64_t seed, uint32_t replica) {
    return {TSU_TAG_DENSE | (replica << 8), (uint32_t)seed, (uint32_t)(seed >> 32)};
}
// R states that advance together in one k2_own launch ([R][n] at states_dev, uniforms [R][n_sweeps][n]), R padded to 2 / 4 / 8
struct OwnGroup {
    int R;
    OwnRep reps[OWN_MAX_R];
    int8_t* states_dev;
};

// The one-launch kernels for d->state (dense_coop.hip), in this order: k2_own; then, natural order only, k2_pipe; then, for a plain
// call, k2_coop.  *out = Done when one of them carried out the call; Declined when none did: the state is then the one at the start of
// the call (a kernel that gave up half way had it restored, and its sticky switch set: this is the one place that sets them).
int tsu_dense_one_launch(tsu_dense* d, const DenseCall& c, DenseOutcome* out);
// owner-computes kernel (dense_own.hip): the call's sweeps of d->state (g == nullptr), natural order or the caller's, or of a group's
// states (natural order; of the call only n_sweeps and uniforms_dev count).  keep: DenseKept::begin_single / begin_group.  *out =
// Declined: nothing was written; GaveUp: the states are half updated.  Writes neither the kept
// fields' bookkeeping nor a switch; it reads one (a group, too, is declined once the single chain's k2_own gave up).
int tsu_dense_own_run(tsu_dense* d, const DenseCall& c, const OwnGroup* g, const DenseResume& keep, DenseOutcome* out);

// dense_plan.h -- the part of a K2 call that is arithmetic on (n, dtype, compute units, order, replicas, sweeps) and the environment:
// which kernel a system goes to, the geometry of the three one-launch kernels, and the state machine of the fields kept from call to
// call.  No HIP in here: a plain C++17 compiler builds it, and tests/host/dense_plan_check.cpp runs it without a GPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#define DB 64            // block of visiting-order positions resolved by one wave
#define SB_SIZE 4096     // positions per superblock of the fixed-point paths (4096 beats 2048 and 8192: profiles/r01_k2_notes.txt)
#define K2W_MAX_SLOTS 3  // slots per lane of the one-wave kernel (fp32; fp64: 2)
#define CO_REFRESH 64    // sweeps between two full recomputations of the fields (bounds floating-point drift)
#define CO_THREADS 1024
#define CO_MAX_N 65536   // bytes of LDS for the staged state vector (phase A)
#define PP_MAXR 24       // rows one streamer wave may own
#define OWN_THREADS 1024
#define OWN_WAVES (OWN_THREADS / 64)
#define OWN_RING 8              // superblocks whose final masks are kept (a workgroup is active at least once per sweep, and cannot be
                                // active before it has applied every earlier superblock: nobody lags more than a sweep = at most
                                // OWN_RING superblocks, checked by the host)
#define OWN_TAG_SPAN 16384u     // generation g of superblock number q carries tag q * SPAN + g + 1 (0 = never written)
#define OWN_MAX_R 8

// an integer switch from the environment (unset: dflt)
static inline int dense_env(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

// ------------------------------------------------------------------------------------------------------------------------ route
// Wave: at most 192 (fp32) / 128 (fp64) sites, one wave with m slots per lane (k2_small); Workgroup: up to 528 / 448 sites, thread per
// site (k2_wg: the measured crossover against the pipeline, tools/archive/dense_mid_times.py); both natural order only.  OneLaunch: from
// 2 DB sites the kernels below (a caller's order too), unless a cooperative launch failed once on this handle (natural_off; natural
// order only) or the call would stage more than 512 MB of orders / uniforms at once.  Blocks: block by block, call by call.
enum class DenseRoute { Wave, Workgroup, OneLaunch, Blocks };
struct DenseRouted {
    DenseRoute route;
    int m;
};
static inline DenseRouted dense_route(int n, bool f64, bool ordered, bool natural_off = false, size_t staged_bytes = 0) {
    const int m = (n + 63) / 64;
    if (!ordered && m <= (f64 ? 2 : K2W_MAX_SLOTS)) return {DenseRoute::Wave, m};
    if (!ordered && n <= (f64 ? 448 : 528)) return {DenseRoute::Workgroup, 0};
    const bool one = n >= 2 * DB && (ordered || !natural_off) && staged_bytes <= ((size_t)1 << 29);
    return {one ? DenseRoute::OneLaunch : DenseRoute::Blocks, 0};
}

// ------------------------------------------------------------------------------------------------------------------------ plans
// takes == false: the kernel declines the call (nothing was written); otherwise the geometry its launch needs.  The LDS opt-in and
// the occupancy query need the runtime and stay with the launch.
struct OwnEnv {
    int use, min_n;  // TSU_K2_OWN, TSU_K2_OWN_MIN: read once per process
    int sb, m;       // TSU_K2_OWN_SB, TSU_K2_OWN_M: read per call (tests vary them)
};
static inline OwnEnv own_env() {
    static const int use = dense_env("TSU_K2_OWN", 1), min_n = dense_env("TSU_K2_OWN_MIN", 2048);
    return {use, min_n, dense_env("TSU_K2_OWN_SB", 0), dense_env("TSU_K2_OWN_M", 0)};
}
struct OwnPlan {
    bool takes;
    int M, R;        // 64 M sites per workgroup; replicas, padded to 1 / 2 / 4 / 8
    int W, G;        // workgroups, 64-site groups
    int sbw, lmax;   // workgroups per superblock, positions per superblock
    int nsb, NP, NA; // superblocks per sweep, groups polled per superblock, accumulators per wave
    int sel;         // k2_own<TJ, M, R, ordered>: 0-2 ordered M = 1, 2, 4; 3-5 natural M = 1, 2, 4; 6-8 natural R = 2, 4, 8
    size_t lds_bytes;
};
static inline OwnPlan own_plan(int n, int cus, bool ord, int R_real, int n_sweeps, const OwnEnv& env) {
    OwnPlan p{};
    if (!env.use || n < env.min_n || n > 65536 || n_sweeps <= 0) return p;
    if (R_real < 1 || R_real > OWN_MAX_R || (ord && R_real != 1)) return p;
    const int R = p.R = R_real == 1 ? 1 : R_real == 2 ? 2 : R_real <= 4 ? 4 : 8;
    int M = 0;
    for (int m = (env.m == 2 || env.m == 4) ? env.m : 1; m <= 4; m *= 2)
        if ((n + 64 * m - 1) / (64 * m) <= cus) {
            M = m;
            break;
        }
    if (!M || (R > 1 && M != 1) || n % 4) return p;  // (rows travel as quads)
    const int RW = 64 * M, W = (n + RW - 1) / RW, G = W * M;
    if (W < 2) return p;
    // superblock: 4096 positions in natural order; a caller's order pays more per generation (every workgroup polls every group and
    // follows every toggle), so fewer, longer fixed points win there: the largest of 16384 / 8192 / 4096 whose toggle list fits the LDS
    // (n = 16384: 0.429 / 0.349 / 0.317 / 0.293 ms per sweep at 2048 / 4096 / 8192 / 16384)
    const int cands[3] = {16384, 8192, 4096};
    p.NA = ord ? 2 : R;
    for (int ci = env.sb > 0 ? 2 : (ord ? 0 : 2); ci < 3; ++ci) {
        int sb = env.sb > 0 ? env.sb : cands[ci];
        if (R > 1 && sb > 4096) sb = 4096;  // (replicas: a deciding wave polls one group per lane)
        if (sb < RW) sb = RW;
        if (sb > 16384) sb = 16384;
        p.sbw = sb / RW;
        if (p.sbw > W) p.sbw = W;
        p.lmax = p.sbw * RW;
        p.nsb = ord ? (n + p.lmax - 1) / p.lmax : (W + p.sbw - 1) / p.sbw;
        p.NP = ord ? G : p.sbw * M;
        p.lds_bytes = ((size_t)8 * (R * G + 2 * R * p.NP) + (size_t)8 * OWN_WAVES * p.NA * M * 64 + (size_t)4 * p.lmax +
                       (size_t)8 * (3 * R + 1) * M * 64 + (ord ? (size_t)2 * n : (R > 1 ? (size_t)R * 64 * 4 : 0)) + 15) / 16 * 16;
        if (p.lds_bytes <= 150 * 1024) break;
    }
    if (!ord && p.nsb > OWN_RING) return p;
    if ((long long)n_sweeps * p.nsb >= (long long)(0xFFFFFFFFu / OWN_TAG_SPAN) - 2) return p;  // generation tags are 32 bits
    if (p.lds_bytes > 150 * 1024) return p;
    p.M = M, p.W = W, p.G = G;
    p.sel = (ord ? 0 : R == 1 ? 3 : 5) + (R > 1 ? (R == 2 ? 1 : R == 4 ? 2 : 3) : (M == 1 ? 0 : M == 2 ? 1 : 2));
    p.takes = true;
    return p;
}

struct PipePlan {
    bool takes, vec;  // vec: rows of J in 16-byte loads
    int sb, ns;       // positions per superblock, solver workgroups
    int grid, u2;     // workgroups; loads in flight per lane on the rows that are not urgent
    size_t lds_bytes;
};
static inline PipePlan pipe_plan(int n, bool f64, int cus) {
    PipePlan p{};
    // superblock: 4096 (2048 for systems that fit one): re-measured on the finished pipeline (profiles/r02_k2_notes.txt) -- 8192,
    // which had won up to n = 12288 half-way through its development, loses everywhere now
    p.sb = n <= 2048 ? 2048 : 4096;
    p.ns = p.sb / 256;
    // small systems: fewer streamer workgroups (every workgroup takes part in the hand-off counters, and a system of a few hundred
    // rows has no work for 4000 waves); from 2048 rows up every CU streams.  128 workgroups per 1024 rows: measured (n = 580 / 1024:
    // 36 / 42 us per sweep; with every CU 46 / 49, with 64 per 1024 rows 40 / 44)
    const int want = p.ns + (int)(((long long)n * 128 + 1023) / 1024);
    p.grid = want < cus ? want : cus;
    // smallest system: 452, just above the one-workgroup kernel (k2_wg: 528 fp32 / 448 fp64 sites): 45-50 us per sweep at
    // n = 580 .. 1020 against 50-62 us on the barrier kernel
    if (n > CO_MAX_N || n < 452 || p.grid < 2 * p.ns) return p;
    if ((long long)(p.grid - p.ns) * (CO_THREADS / 64) * PP_MAXR < n) return p;
    if (n % 4) return p;  // state / flips travel as dwords
    p.vec = n % (f64 ? 2 : 4) == 0;
    // ONE load in flight while the rows that are not urgent take less time than the solvers' latency-bound iterations anyway
    // (N = 16384: 0.386 -> 0.353 ms per sweep; profiles/r02_k2_notes.txt), eight once the strips dominate
    p.u2 = n <= 20480 ? 1 : 8;
    p.lds_bytes = (size_t)((n > p.sb ? n : p.sb) + 15) / 16 * 16;
    p.takes = true;
    return p;
}

struct CoopPlan {
    bool takes, vec;
    int grid, nsb;
    size_t lds_bytes;
};
static inline CoopPlan coop_plan(int n, bool f64, int cus) {
    CoopPlan p{};
    if (n > CO_MAX_N) return p;  // the staged state vector must fit in LDS: larger systems take the block-by-block path
    p.vec = n % (f64 ? 2 : 4) == 0;
    p.lds_bytes = (size_t)((n > SB_SIZE ? n : SB_SIZE) + 15) / 16 * 16;
    p.nsb = (n + SB_SIZE - 1) / SB_SIZE;
    // one workgroup per CU: every phase is either a stream (16 waves x 8 loads in flight per CU) or tiny, and fewer
    // arrivals make a cheaper barrier; small systems use fewer workgroups still
    const int useful = (n + CO_THREADS / 64 - 1) / (CO_THREADS / 64);
    p.grid = cus < useful ? cus : useful;
    p.takes = true;
    return p;
}

// ------------------------------------------------------------------------------------------------------------------ kept fields
enum class DenseOutcome { Declined, Done, GaveUp };  // GaveUp: the kernel ran and left its states half updated
struct DenseResume {
    int resume;       // the kept fields are those of the state the call starts from: no pass over J to rebuild them
    int refresh_off;  // sweeps since they were last computed from scratch, at the start of the call
    int persist;      // leave the fields of the final state(s) behind
    int was_valid, streak;  // (single chain) fields_valid and pipe_streak as begin_single found them: end_single's
};

// The fields f = J s + b that the one-launch kernels hand from call to call (a loop of one-sweep calls -- annealing, tempering -- would
// otherwise stream J once more per call to rebuild them, and an energy once more again), and the three sticky switches of a handle.
struct DenseKept {
    // the single chain: d->co_fields
    int fields_valid;   // they belong to d->state (forget() on everything else that writes the state)
    int since_refresh;  // sweeps since they were last computed from scratch (CO_REFRESH bounds the drift across calls too)
    int pipe_streak;    // consecutive one-launch calls on this state: the second one starts to keep the fields
    // a group of up to eight replicas (a tempering loop is a loop of short calls on states that come back unchanged or swapped)
    double* rep_fields[2];  // device, [8][n] each: the rows of the states the last group returned (in rep_cur), and where the next writes
    int8_t* rep_prev;       // host copy of those states [8][n]: an incoming state is matched against them byte for byte
    int rep_prev_n;         // how many there are: only end_group sets it, after a launch that wrote their rows
    int rep_cur, rep_since;
    int rep_match;          // the resident state IS row rep_match - 1 (tsu_dense_set_state; 0: no)
    // set by the single-chain driver (tsu_dense_one_launch), never cleared
    int own_failed;   // k2_own ran and gave up half way
    int pp_failed;    // k2_pipe ran and gave up half way
    int co_disabled;  // cooperative launch unavailable or failed once: natural-order calls skip the one-launch kernels

    // something other than a one-launch kernel's successful call writes (or is about to write) d->state
    void forget() { fields_valid = rep_match = pipe_streak = 0; }
    // row of the kept replica states that equals `s` byte for byte (looked for from row `first` on, cyclically), or -1
    int find(const int8_t* s, size_t n, int first = 0) const {
        for (int t = 0; t < rep_prev_n; ++t) {
            const int p = (first + t) % rep_prev_n;
            if (memcmp(s, rep_prev + (size_t)p * n, n) == 0) return p;
        }
        return -1;
    }
    double* rep_in() const { return rep_fields[rep_cur]; }  // (nullptr: no buffers, and then no rows)
    double* rep_out() const { return rep_fields[rep_cur ^ 1]; }
    bool own_usable() const { return !own_failed; }
    bool natural_off() const { return co_disabled != 0; }
    void match_state(const int8_t* s, size_t n) { rep_match = find(s, n) + 1; }
    int matched_row() const { return rep_match <= rep_prev_n ? rep_match - 1 : -1; }

    // A one-launch call on d->state: resume when the previous call left the fields for exactly this state and no refresh is due; keep
    // them from the second consecutive call on (a lone call does not pay for rows it would not need again).  Whatever happens next,
    // they stop being valid until a kernel's end_single(Done).
    DenseResume begin_single() {
        const int resume = fields_valid && since_refresh % CO_REFRESH != 0;
        const DenseResume r = {resume, resume ? since_refresh : 0, pipe_streak >= 1, fields_valid, pipe_streak};
        forget();
        return r;
    }
    // ... and the next kernel of the same call begins from what this one found, minus the validity after a give-up
    void end_single(DenseOutcome o, const DenseResume& r, int n_sweeps) {
        pipe_streak = r.streak + (o == DenseOutcome::Done);
        fields_valid = o == DenseOutcome::Done ? r.persist : o == DenseOutcome::Declined && r.was_valid;
        if (o == DenseOutcome::Done) since_refresh = (r.refresh_off + n_sweeps) % CO_REFRESH;
    }
    // A group of m replicas (padded to mp: the padding repeats the first); keep: the call has at most eight, and rep_fields and rep_prev
    // exist.  src[q]: the kept row of incoming state q or -1.  A state that comes back byte for byte as one of those the last group
    // returned (in any position: tempering swaps them) resumes from that state's fields.
    DenseResume begin_group(const int8_t* states, size_t n, int m, int mp, bool keep, int* src) {
        rep_match = 0;  // (the kept rows are about to change)
        bool all_known = keep && rep_prev_n > 0;
        for (int q = 0; q < mp; ++q) {
            src[q] = keep ? find(states + (size_t)(q < m ? q : 0) * n, n, q) : -1;
            all_known = all_known && src[q] >= 0;
        }
        const int resume = all_known && rep_since % CO_REFRESH != 0;
        return {resume, resume ? rep_since : 0, keep, 0, 0};
    }
    // states: the m states the launch returned.  Rows are recorded only from a launch that wrote them (Done with r.persist); one that
    // declined or gave up leaves none, one that did not persist leaves the earlier rows (still the fields of their states)
    void end_group(DenseOutcome o, const DenseResume& r, int n_sweeps, const int8_t* states, size_t n, int m) {
        if (o != DenseOutcome::Done) rep_prev_n = 0;
        if (o != DenseOutcome::Done || !r.persist) return;
        rep_since = (r.refresh_off + n_sweeps) % CO_REFRESH;
        rep_cur ^= 1;
        memcpy(rep_prev, states, (size_t)m * n);
        rep_prev_n = m;
    }
};

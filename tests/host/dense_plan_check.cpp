// dense_plan_check.cpp -- the arithmetic of a K2 call (csrc/dense_plan.h) without a GPU: routes, the plans of the three one-launch
// kernels and the kept-field state machine.  One line per case; the exit status is the number of failed cases (tests/test_dense_plan_cpu.py).
#include <cstdio>
#include <vector>

#include "dense_plan.h"

static int failures = 0;
#define CHECK(what, cond)                                        \
    do {                                                         \
        const bool ok__ = (cond);                                \
        printf("%s  %s\n", ok__ ? "ok  " : "FAIL", what);        \
        failures += !ok__;                                       \
    } while (0)

static const int CUS = 256;
static const OwnEnv ENV = {1, 2048, 0, 0};

static bool routed(int n, bool f64, bool ordered, DenseRoute want, int m = 0) {
    const DenseRouted r = dense_route(n, f64, ordered);
    return r.route == want && r.m == m;
}
static OwnPlan own(int n, bool ord = false, int R = 1, int n_sweeps = 1, OwnEnv env = ENV) { return own_plan(n, CUS, ord, R, n_sweeps, env); }

static void check_route() {
    CHECK("route fp32 12: one wave, m = 1", routed(12, false, false, DenseRoute::Wave, 1));
    CHECK("route fp32 192: one wave, m = 3", routed(192, false, false, DenseRoute::Wave, 3));
    for (int n : {193, 200, 528}) CHECK("route fp32 193 / 200 / 528: one workgroup", routed(n, false, false, DenseRoute::Workgroup));
    for (int n : {529, 580}) CHECK("route fp32 529 / 580: one launch", routed(n, false, false, DenseRoute::OneLaunch));
    CHECK("route fp64 128: one wave, m = 2", routed(128, true, false, DenseRoute::Wave, 2));
    for (int n : {129, 448}) CHECK("route fp64 129 / 448: one workgroup", routed(n, true, false, DenseRoute::Workgroup));
    CHECK("route fp64 449: one launch", routed(449, true, false, DenseRoute::OneLaunch));
    for (bool f64 : {false, true}) {
        CHECK("route ordered 12 / 127: block by block", routed(12, f64, true, DenseRoute::Blocks) && routed(127, f64, true, DenseRoute::Blocks));
        CHECK("route ordered 128 / 580: one launch", routed(128, f64, true, DenseRoute::OneLaunch) && routed(580, f64, true, DenseRoute::OneLaunch));
    }
    CHECK("route: a failed cooperative launch takes natural order block by block, not a caller's order, not the small kernels",
          dense_route(2048, false, false, true).route == DenseRoute::Blocks && dense_route(2048, false, true, true).route == DenseRoute::OneLaunch &&
              dense_route(200, false, false, true).route == DenseRoute::Workgroup);
    CHECK("route: 512 MB of staged inputs stay one launch, a byte more goes call by call",
          dense_route(2048, false, true, false, (size_t)1 << 29).route == DenseRoute::OneLaunch &&
              dense_route(2048, false, true, false, ((size_t)1 << 29) + 1).route == DenseRoute::Blocks);
}

static void check_own() {
    CHECK("own 2044 declines (below own_min)", !own(2044).takes);
    for (bool ord : {false, true}) CHECK("own 2048 and 4100 are taken, ordered and natural", own(2048, ord).takes && own(4100, ord).takes);
    CHECK("own 2051 declines (n % 4)", !own(2051).takes);
    // (natural order keeps OWN_RING superblocks of 4096: 32768 sites; beyond, up to the limit of 65536, with superblocks of 8192)
    CHECK("own 32768 is taken, 32772 and 65536 decline (more than OWN_RING superblocks)", own(32768).takes && own(32768).nsb == 8 && !own(32772).takes && !own(65536).takes);
    CHECK("own 65536 is taken with superblocks of 8192, 65540 declines", own(65536, false, 1, 1, {1, 2048, 8192, 0}).takes && own(65536, false, 1, 1, {1, 2048, 8192, 0}).M == 4 &&
                                                                             !own(65540, false, 1, 1, {1, 2048, 8192, 0}).takes && !own(65540).takes);
    const OwnPlan a = own(16384), b = own(16384, true);
    CHECK("own 16384 natural: M = 1, W = 256, superblocks of 4096, nsb = 4", a.takes && a.M == 1 && a.W == 256 && a.lmax == 4096 && a.nsb == 4 && a.sel == 3);
    CHECK("own 16384 ordered: one superblock of 16384", b.takes && b.lmax == 16384 && b.nsb == 1 && b.sel == 0);
    CHECK("own R = 3 pads to 4, 5 to 8, 9 declines", own(4096, false, 3).R == 4 && own(4096, false, 3).sel == 7 && own(4096, false, 5).R == 8 &&
                                                         own(4096, false, 5).takes && !own(4096, false, 9).takes);
    CHECK("own R > 1 with an order declines", !own(4096, true, 2).takes);
    CHECK("own: use = 0 and n_sweeps = 0 decline", !own(4096, false, 1, 1, {0, 2048, 0, 0}).takes && !own(4096, false, 1, 0).takes);
    setenv("TSU_K2_OWN_SB", "8192", 1);
    const OwnPlan s = own(16384, false, 1, 1, own_env());
    unsetenv("TSU_K2_OWN_SB");
    setenv("TSU_K2_OWN_M", "2", 1);
    const OwnPlan m = own(16384, false, 1, 1, own_env());
    unsetenv("TSU_K2_OWN_M");
    CHECK("own TSU_K2_OWN_SB=8192 is honoured", s.takes && s.lmax == 8192 && s.nsb == 2);
    CHECK("own TSU_K2_OWN_M=2 is honoured", m.takes && m.M == 2 && m.W == 128 && m.G == 256 && m.sel == 4);
    CHECK("own: the overrides are read per call", own(16384, false, 1, 1, own_env()).lmax == 4096 && own(16384, false, 1, 1, own_env()).M == 1);
    const long long tags = (long long)(0xFFFFFFFFu / OWN_TAG_SPAN) - 2;  // (n_sweeps * nsb must stay below)
    CHECK("own declines once the generation tags would overflow", own(16384, false, 1, (int)((tags - 1) / 4)).takes && !own(16384, false, 1, (int)((tags + 3) / 4)).takes);
    bool fits = true;
    for (int n = 2048; n <= 65536; n += 1028)
        for (int R : {1, 2, 4, 8})
            for (bool ord : {false, true}) {
                const OwnPlan p = own(n, ord, R);
                fits = fits && (!p.takes || p.lds_bytes <= 150 * 1024);
            }
    CHECK("own: every taken plan's LDS is at most 150 KiB", fits);
}

static void check_pipe_coop() {
    const PipePlan p452 = pipe_plan(452, false, CUS), p580 = pipe_plan(580, false, CUS);
    CHECK("pipe 448 declines", !pipe_plan(448, false, CUS).takes);
    CHECK("pipe 452 is taken, grid 8 + 57", p452.takes && p452.ns == 8 && p452.grid == 8 + 57);
    CHECK("pipe 580 is taken, grid 8 + 73", p580.takes && p580.grid == 8 + 73);
    CHECK("pipe 2047 declines (n % 4)", !pipe_plan(2047, false, CUS).takes);
    CHECK("pipe 2048: superblocks of 2048", pipe_plan(2048, false, CUS).takes && pipe_plan(2048, false, CUS).sb == 2048 && pipe_plan(2048, false, CUS).grid == CUS);
    CHECK("pipe 4096: superblocks of 4096, U2 = 1", pipe_plan(4096, false, CUS).sb == 4096 && pipe_plan(4096, false, CUS).u2 == 1);
    CHECK("pipe 20480: U2 = 1; 20484: U2 = 8", pipe_plan(20480, false, CUS).u2 == 1 && pipe_plan(20484, false, CUS).takes && pipe_plan(20484, false, CUS).u2 == 8);
    CHECK("pipe 65540 declines", pipe_plan(65536, false, CUS).takes && !pipe_plan(65540, false, CUS).takes);
    // (grid < 2 ns: sixteen solver workgroups at n > 2048; at n <= 2048 there are eight, and sixteen compute units just suffice)
    CHECK("pipe on 16 compute units declines (grid < 2 ns)", !pipe_plan(4096, false, 16).takes && !pipe_plan(2048, false, 15).takes && pipe_plan(2048, false, 16).takes);
    CHECK("pipe vec: rows in 16-byte loads", pipe_plan(2050 + 2, true, CUS).vec && pipe_plan(2052, false, CUS).vec && !pipe_plan(4100 + 2, false, CUS).takes);
    const CoopPlan c = coop_plan(2051, true, CUS);
    CHECK("coop 2051 fp64 is taken: scalar loads, one superblock, LDS of 4096", c.takes && !c.vec && c.nsb == 1 && c.lds_bytes == 4096);
    CHECK("coop 65537 declines", coop_plan(65536, true, CUS).takes && !coop_plan(65537, true, CUS).takes);
    CHECK("coop grid = min(cus, ceil(n / 16))", c.grid == 129 && coop_plan(8192, false, CUS).grid == CUS && coop_plan(8192, false, 64).grid == 64);
}

static void check_kept() {
    DenseKept k{};
    DenseResume r = k.begin_single();
    CHECK("kept: the first call neither resumes nor persists", !r.resume && !r.persist && !k.fields_valid);
    k.end_single(DenseOutcome::Done, r, 1);
    r = k.begin_single();
    CHECK("kept: the second call persists", !r.resume && r.persist);
    k.end_single(DenseOutcome::Done, r, 1);
    CHECK("kept: ... and leaves valid fields", k.fields_valid && k.since_refresh == 1);
    r = k.begin_single();
    CHECK("kept: the third call resumes", r.resume && r.refresh_off == 1 && r.persist);
    k.end_single(DenseOutcome::Done, r, CO_REFRESH - 1);
    CHECK("kept: since wraps at CO_REFRESH", k.since_refresh == 0 && k.fields_valid);
    r = k.begin_single();
    CHECK("kept: a resume is refused at the wrap", !r.resume && r.refresh_off == 0 && r.persist);
    // one call, two kernels: a kernel that declines hands the next what it found; one that gives up, all but the validity
    k.end_single(DenseOutcome::Declined, r, 5);
    DenseResume r2 = k.begin_single();
    CHECK("kept: a decline hands the next kernel the same start", r2.persist && r2.was_valid && r2.streak == r.streak && k.since_refresh == 0);
    k.end_single(DenseOutcome::Done, r2, 3);
    r = k.begin_single();
    k.end_single(DenseOutcome::GaveUp, r, 3);
    r2 = k.begin_single();
    CHECK("kept: a give-up hands the next kernel the streak, not the fields", r.resume && !r2.resume && r2.persist);
    k.end_single(DenseOutcome::Done, r2, 3);
    CHECK("kept: ... and the call that follows resumes again", k.begin_single().resume);

    // replicas: 4 rows of n = 16 bytes
    const size_t n = 16;
    std::vector<int8_t> prev(8 * n), st(8 * n), out(8 * n);
    for (size_t i = 0; i < 8 * n; ++i) st[i] = (int8_t)(i % n < i / n + 5), out[i] = (int8_t)((i / n + i % n / (i / n + 1)) % 2);
    k.rep_prev = prev.data();
    k.fields_valid = 1, k.pipe_streak = 2, k.since_refresh = 7;
    int src[8];
    DenseResume g = k.begin_group(st.data(), n, 4, 4, true, src);
    CHECK("kept: a first group persists, knows no row", !g.resume && g.persist && src[0] == -1 && src[3] == -1);
    k.end_group(DenseOutcome::Done, g, 2, out.data(), n, 4);
    CHECK("kept: ... and records its rows", k.rep_prev_n == 4 && k.rep_cur == 1 && k.rep_since == 2);
    CHECK("kept: a group leaves the single chain's state alone", k.fields_valid == 1 && k.pipe_streak == 2 && k.since_refresh == 7);
    CHECK("kept: find returns the row", k.find(out.data() + 2 * n, n) == 2 && k.find(st.data(), n) == -1);
    std::vector<int8_t> twin(out);
    memcpy(twin.data() + 3 * n, twin.data() + 1 * n, n);  // (rows 1 and 3 equal)
    memcpy(k.rep_prev, twin.data(), 4 * n);
    CHECK("kept: find looks at a row's own position first, then the others", k.find(twin.data() + n, n, 3) == 3 && k.find(twin.data() + n, n, 1) == 1 &&
                                                                               k.find(twin.data() + n, n, 2) == 3 && k.find(twin.data() + n, n, 0) == 1);
    twin[n + 5] ^= 1;
    CHECK("kept: find finds nothing after one byte is edited", k.find(twin.data() + n, n) == -1 && k.find(twin.data() + 3 * n, n) == 1);
    memcpy(k.rep_prev, out.data(), 4 * n);
    // the states come back swapped: every one is known, the group resumes
    std::vector<int8_t> sw(out);
    memcpy(sw.data(), out.data() + n, n);
    memcpy(sw.data() + n, out.data(), n);
    k.match_state(out.data() + 3 * n, n);
    CHECK("kept: set_state matches a kept row", k.matched_row() == 3);
    g = k.begin_group(sw.data(), n, 3, 4, true, src);
    CHECK("kept: swapped states resume from their rows (the padding repeats the first)", g.resume && g.refresh_off == 2 && src[0] == 1 && src[1] == 0 && src[2] == 2 && src[3] == 1 && k.matched_row() == -1);
    k.forget();
    CHECK("kept: forget clears validity, match and streak, not the replica rows", !k.fields_valid && !k.pipe_streak && k.matched_row() == -1 && k.rep_prev_n == 4);
    DenseKept done_not_persisted = k;
    done_not_persisted.end_group(DenseOutcome::Done, {0, 0, 0, 0, 0}, 2, st.data(), n, 4);
    CHECK("kept: a group that is done but did not persist records no rows", done_not_persisted.rep_prev_n == 4 && done_not_persisted.rep_cur == 1 &&
                                                                                done_not_persisted.find(st.data(), n) == -1 && memcmp(prev.data(), out.data(), 4 * n) == 0);
    for (DenseOutcome o : {DenseOutcome::GaveUp, DenseOutcome::Declined}) {
        DenseKept f = k;
        f.fields_valid = 1, f.pipe_streak = 3, f.own_failed = 0;
        f.end_group(o, g, 2, nullptr, n, 0);
        CHECK("kept: a group that gave up / declined leaves zero rows and the single chain's sticky state alone",
              f.rep_prev_n == 0 && f.find(out.data(), n) == -1 && f.matched_row() == -1 && f.fields_valid == 1 && f.pipe_streak == 3 && !f.own_failed && !f.pp_failed && !f.co_disabled);
    }
    g = k.begin_group(out.data(), n, 4, 4, true, src);
    k.end_group(DenseOutcome::Done, g, CO_REFRESH - 2, out.data(), n, 4);
    CHECK("kept: the group's since wraps at CO_REFRESH, and a resume is refused there", k.rep_since == 0 && !k.begin_group(out.data(), n, 4, 4, true, src).resume && src[2] == 2);
    // a call of nine or more replicas (keep == false) keeps nothing
    DenseKept big{};
    big.rep_prev = prev.data();
    g = big.begin_group(st.data(), n, 8, 8, false, src);
    big.end_group(DenseOutcome::Done, g, 1, st.data(), n, 8);
    CHECK("kept: a call of 9 or more replicas keeps nothing", !g.persist && !g.resume && src[0] == -1 && big.rep_prev_n == 0 && big.rep_cur == 0);
}

int main() {
    check_route();
    check_own();
    check_pipe_coop();
    check_kept();
    printf("%d failed\n", failures);
    return failures;
}

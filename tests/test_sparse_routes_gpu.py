"""K5's update routes beyond the degree-2 chain (-m gpu).  Every case first asserts its PLAN (SparseSystem.plan(): which kernel each
colour class takes, tests/helpers/sparse_plan_twin.py has the literals) and then compares the bits with the oracle's sequential loop
on the same CSR rows and order: degrees 1 to 4, site strides 1, 2, 3 and -2, three regular classes, pairs whose classes differ in
degree, coupling and bias, end bands of up to 64 rows, a generic class next to a stencil class, a second class one longer than the
first, saturated thresholds, the replica argument, and draws whose leading 27 bits EQUAL a threshold's (built, not forced)."""
import functools
import importlib.util
import os

import numpy as np
import pytest

from oracle import oracle as ora

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("sparse_plan_twin", os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers",
                                                                                "sparse_plan_twin.py"))
twin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(twin)

# n = 40008: the second class starts at 20004, a multiple of 4 (k5_stencil4); 40010: at 20005 (k5_stencil1, for both classes of a pair).
# The strip's classes are regular at any size, but at 30000 / 30006 sites the whole system runs on k5_small (<= 32768); 60000 and
# 60006 (classes at 20002, 40004) put its three classes of stride 3 on the stencil kernels.
TABLE = ([(g, n) for g in ("dimers", "degree3", "degree4", "asymmetric", "halves") for n in (40008, 40010)]
         + [("strip", 30000), ("strip", 30006), ("strip", 60000), ("strip", 60006)]
         + [(g, 40008) for g in ("chain_first38", "chain_first64", "chain_first65", "chain_both_ends", "chain_interior", "chain_descending")]
         + [("chain_odd_first", 40009)])
T1, T2, T3, SEED = 1.1, 0.4, 2.5, 17


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    from tsu import _hip
    _hip.Context.default()


@functools.lru_cache(maxsize=None)
def _graph(name, n):
    return twin.graph(name, n)


@functools.lru_cache(maxsize=None)
def _reference(name, n):
    """The oracle's states of the run every table case makes (the switches do not enter): start, after sweep(T1, 3), after
    sweep(T2, 2), and the two samples of sample(T3, burn-in 0, 1 sweep apart, 2 samples).  Seven sweeps, counters continuing."""
    A, bias, _, order, _, _ = _graph(name, n)
    st = np.random.default_rng(n).integers(0, 2, size=n).astype(np.int8)
    a = ora.sparse_sweep_philox(st, A.indptr, A.indices, A.data, bias, T1, 3, SEED, sweep0=3, order=order)
    b = ora.sparse_sweep_philox(a, A.indptr, A.indices, A.data, bias, T2, 2, SEED, sweep0=6, order=order)
    s0 = ora.sparse_sweep_philox(b, A.indptr, A.indices, A.data, bias, T3, 1, SEED, sweep0=8, order=order)
    s1 = ora.sparse_sweep_philox(s0, A.indptr, A.indices, A.data, bias, T3, 1, SEED, sweep0=9, order=order)
    return st, a, b, s0, s1


def _system(A, bias, offsets, order):
    from tsu import _hip
    return _hip.SparseSystem(A.indptr, A.indices, A.data, bias, offsets, order)


@pytest.mark.parametrize("name,n", TABLE)
@pytest.mark.parametrize("pair,tie", [(1, 0), (0, 0), (1, 1), (0, 1)])
def test_route_plan_then_bits(name, n, pair, tie, monkeypatch):
    monkeypatch.setenv("TSU_K5_PAIR", str(pair))
    monkeypatch.setenv("TSU_K5_TEST_TIE", str(tie))
    for k in ("TSU_K5_STENCIL", "TSU_K5_V4"):
        monkeypatch.delenv(k, raising=False)
    A, bias, offsets, order, classes, pairs = _graph(name, n)
    st, a, b, s0, s1 = _reference(name, n)
    g = _system(A, bias, offsets, order)
    plan = g.plan()
    assert plan == twin.expected_plan(offsets, classes, pairs, use_pairs=bool(pair))
    assert plan == twin.classify(A.indptr, A.indices, A.data, bias, offsets, order, use_pairs=bool(pair))
    g.set_state(st)
    g.sweep(T1, 3, seed=SEED, sweep0=3)
    np.testing.assert_array_equal(g.get_state(), a)
    g.sweep(T2, 2, seed=SEED, sweep0=6)
    np.testing.assert_array_equal(g.get_state(), b)
    got = g.sample(T3, 0, 1, 2, seed=SEED, sweep0=8)
    np.testing.assert_array_equal(got[0], s0, err_msg="sample 0")
    np.testing.assert_array_equal(got[1], s1, err_msg="sample 1")
    g.close()


def test_the_plans_cover_every_route():
    """What the cases above assert, taken together (literals, no GPU work): degrees 1 to 4, strides 1, 2, 3 and -2, pair 0, 1, 2,
    v4 0 and 1, lo 38 and 64, hi 61, and a generic class next to a stencil class."""
    recs, mixed = [], False
    for name, n in TABLE:
        _, _, offsets, _, classes, pairs = _graph(name, n)
        plan = twin.expected_plan(offsets, classes, pairs)
        recs += [r for r in plan if r["route"] == 1]
        mixed = mixed or sorted(r["route"] for r in plan) == [0, 1]
    for key, values in (("deg", (1, 2, 3, 4)), ("site_stride", (1, 2, 3, -2)), ("pair", (0, 1, 2)), ("v4", (0, 1)), ("lo", (38, 64)), ("hi", (61,))):
        assert set(values) <= {r[key] for r in recs}, key
    assert mixed


@pytest.mark.parametrize("n,route", [(4099, 2), (40008, 1)])
def test_replica_argument(n, route):
    """replica = 3 enters the Philox counter's tag word: the oracle's replica = 3, and not the bits of replica 0."""
    A, bias, offsets, order, _, _ = _graph("chain", n)
    st = np.random.default_rng(n).integers(0, 2, size=n).astype(np.int8)
    g = _system(A, bias, offsets, order)
    assert [r["route"] for r in g.plan()] == [route, route]
    g.set_state(st)
    g.sweep(T1, 3, seed=SEED, sweep0=2, replica=3)
    want = ora.sparse_sweep_philox(st, A.indptr, A.indices, A.data, bias, T1, 3, SEED, sweep0=2, replica=3, order=order)
    np.testing.assert_array_equal(g.get_state(), want)
    assert (want != ora.sparse_sweep_philox(st, A.indptr, A.indices, A.data, bias, T1, 3, SEED, sweep0=2, order=order)).any()
    got = g.sample(T2, 1, 1, 2, seed=SEED, sweep0=5, replica=3)
    want = ora.sparse_sweep_philox(want, A.indptr, A.indices, A.data, bias, T2, 2, SEED, sweep0=5, replica=3, order=order)
    np.testing.assert_array_equal(got[0], want)
    want = ora.sparse_sweep_philox(want, A.indptr, A.indices, A.data, bias, T2, 1, SEED, sweep0=7, replica=3, order=order)
    np.testing.assert_array_equal(got[1], want)
    g.close()


@pytest.mark.parametrize("b,present", [(-1.6, (True, True, True)), (1.6, (False, False, True))])
def test_saturated_thresholds(b, present, monkeypatch):
    """Degree 4, Jv = 0.8, T = 0.03.  Bias -1.6: the fields -1.6, -0.8, 0, 0.8, 1.6 over T are -53, -27, 0, 27, 53 -- the sigmoid's
    clamp at +-20 gives p = 0 (threshold 0), 1/2 and p = 1 (threshold 2^53) in one run.  Bias +1.6: every count is clamped to p = 1."""
    for k in ("TSU_K5_PAIR", "TSU_K5_TEST_TIE", "TSU_K5_STENCIL", "TSU_K5_V4"):
        monkeypatch.delenv(k, raising=False)
    n, T = 40008, 0.03
    A, _, offsets, order, classes, pairs = _graph("degree4", n)
    bias = np.full(n, b)
    thr = twin.thresholds(4, 0.8, b, T, ora.c_sigmoid)
    assert (0 in thr, any(0 < t < 1 << 53 for t in thr), 1 << 53 in thr) == present, thr
    st = np.random.default_rng(4).integers(0, 2, size=n).astype(np.int8)
    g = _system(A, bias, offsets, order)
    assert g.plan() == twin.expected_plan(offsets, classes, pairs)
    g.set_state(st)
    g.sweep(T, 3, seed=SEED, sweep0=1)
    want = ora.sparse_sweep_philox(st, A.indptr, A.indices, A.data, bias, T, 3, SEED, sweep0=1, order=order)
    np.testing.assert_array_equal(g.get_state(), want)
    if b > 0:
        assert want.all()
    else:
        assert 0 < want.sum() < n
    g.close()


# ------------------------------------------------------------------ real ties

TIE_T, TIE_SEED, TIE_SWEEP = 0.9, 23, 5


def _draw(site):
    """The 53 bits of the site's uniform in the first sweep of the call."""
    m = ora.dense_uniform(site, TIE_SWEEP, TIE_SEED) * 9007199254740992.0
    assert m == int(m)
    return int(m)


def _tie_bias(cnt, target):
    """Bisect a class bias until the oracle's own threshold expression for `cnt` set neighbours lies within 2^10 of `target`."""
    lo, hi = -40.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        t = twin.thresholds(2, 0.8, mid, TIE_T, ora.c_sigmoid)[cnt]
        if abs(t - target) <= 1 << 10:
            return mid, t
        lo, hi = (mid, hi) if t < target else (lo, mid)
    raise AssertionError("the bisection did not converge")


@pytest.mark.parametrize("which", ["own", "code"])
@pytest.mark.parametrize("side", [1, -1])
def test_real_tie_in_one_wave(which, side, monkeypatch):
    """The chain at n = 40008 (paired, four positions per thread), TSU_K5_TEST_TIE = 0: ONE wave of the first class's launch meets a
    draw whose leading 27 bits equal a threshold's, all others take the 27-bit compares.  own: a regular site of the first class and
    its own threshold (a == ta); code: a regular site of the second class, whose decision by neighbour count the first class's launch
    prepares (a2 == tho[cnt], cnt taken from the oracle after the first class's update).  The class's bias is bisected until the
    threshold lies 2^22 above the draw (side = 1: the site must become 1, a compare of the leading bits alone says 0) or 2^22 below
    (side = -1: it must become 0).  The margin of 2^22 keeps a few-ulp difference between the device's and the host's exp from
    moving the tie; 2^26 boundaries between draw and threshold are excluded by the choice of the site."""
    monkeypatch.setenv("TSU_K5_TEST_TIE", "0")
    for k in ("TSU_K5_PAIR", "TSU_K5_STENCIL", "TSU_K5_V4"):
        monkeypatch.delenv(k, raising=False)
    n = 40008
    A, bias, offsets, order, classes, pairs = _graph("chain", n)
    bias = bias.copy()
    st = np.random.default_rng(n).integers(0, 2, size=n).astype(np.int8)
    low = (1 << 26) - 1
    # a site in the middle of its class (far from the end rows' threads) whose draw has room for 2^22 + 2^10 on either side
    site = next(i for i in range(20000 + (which == "code"), 30000, 2) if 1 << 23 <= (_draw(i) & low) <= (1 << 26) - (1 << 23))
    m = _draw(site)
    if which == "own":   # the first class reads the start state
        cnt = int(st[site - 1] + st[site + 1])
    else:                # the second class reads what the first class's update left: independent of the second class's bias
        one = ora.sparse_sweep_philox(st, A.indptr, A.indices, A.data, bias, TIE_T, 1, TIE_SEED, sweep0=TIE_SWEEP, order=order)
        cnt = int(one[site - 1] + one[site + 1])
    b, thr = _tie_bias(cnt, m + side * (1 << 22))
    bias[order[offsets[site & 1]:offsets[(site & 1) + 1]]] = b
    # the construction holds: equal leading 27 bits, the offset, no 2^26 boundary in between
    assert thr >> 26 == m >> 26 and abs(abs(thr - m) - (1 << 22)) <= 1 << 10 and (thr > m) == (side > 0)
    assert twin.thresholds(2, 0.8, b, TIE_T, ora.c_sigmoid)[cnt] == thr
    want = ora.sparse_sweep_philox(st, A.indptr, A.indices, A.data, bias, TIE_T, 1, TIE_SEED, sweep0=TIE_SWEEP, order=order)
    assert int(want[site - 1] + want[site + 1]) == cnt or which == "own"
    assert want[site] == (1 if side > 0 else 0)
    g = _system(A, bias, offsets, order)
    plan = g.plan()
    assert plan == twin.expected_plan(offsets, classes, pairs)
    assert [(r["pair"], r["v4"]) for r in plan] == [(1, 1), (2, 1)]
    g.set_state(st)
    g.sweep(TIE_T, 1, seed=TIE_SEED, sweep0=TIE_SWEEP)
    got = g.get_state()
    assert got[site] == want[site], (site, cnt, m, thr)
    np.testing.assert_array_equal(got, want)
    g.sweep(TIE_T, 2, seed=TIE_SEED, sweep0=TIE_SWEEP + 1)
    want = ora.sparse_sweep_philox(want, A.indptr, A.indices, A.data, bias, TIE_T, 2, TIE_SEED, sweep0=TIE_SWEEP + 1, order=order)
    np.testing.assert_array_equal(g.get_state(), want)
    g.close()

"""K5 walker batches on the GPU (-m gpu): every walker is the single handle and the oracle bit for bit, a tempering run is the NumPy
twin (tests/helpers/sparse_batch_twin.py), the energies are fixed-order sums (the same bits on every run, on both routes and in the
twin), best states, anneal, the launch counts of both routes, and GibbsSampler.parallel_tempering on a sparse graph."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle as ora
from test_sparse_cpu import random_graph  # (tests/ is on sys.path: rootdir conftest, prepend import mode)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("sparse_batch_twin", os.path.join(HERE, "helpers", "sparse_batch_twin.py"))
twin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(twin)

K5S_MAX = 32768
ROUTES = ["small", "colour"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    from tsu import _hip
    _hip.Context.default()


def _route(monkeypatch, route, n):
    """Select the route (a graph above K5S_MAX has the colour route only)."""
    assert route == "colour" or n <= K5S_MAX
    if route == "colour":
        monkeypatch.setenv("TSU_K5B_SMALL", "0")
    else:
        monkeypatch.delenv("TSU_K5B_SMALL", raising=False)


@functools.lru_cache(maxsize=None)
def _graph(name):
    """(A, bias) of a named test graph, Gaussian couplings."""
    from tsu.graph import canonical_csr
    if name == "one":
        A = canonical_csr(sp.csr_matrix(np.array([[0.7]])))
    elif name == "chain7":
        A = canonical_csr(sp.diags([np.full(6, 0.8), np.full(6, 0.8)], [1, -1]))
    elif name == "g64":
        A = random_graph(64, 0.08, 64)
    elif name == "g200":
        A = random_graph(200, 0.03, 200)  # self-loops on 20 % of the sites, some isolated sites
    else:
        n = int(name[1:])
        A = random_graph(n, 3.0 / n, n)
    return A, np.random.default_rng(A.shape[0]).normal(size=A.shape[0])


@functools.lru_cache(maxsize=None)
def _dyadic(n, seed):
    """A sparse system whose energies are exact in every summation order (oracle.dyadic_system under a symmetric mask)."""
    from tsu.graph import canonical_csr
    J, b, _ = ora.dyadic_system(n, seed)
    keep = np.triu(np.random.default_rng(seed).random((n, n)) < min(1.0, 6.0 / n))
    A = canonical_csr(sp.csr_matrix(J * (keep | keep.T)))
    assert ora.energy_is_exact(A.toarray(), b)
    return A, b


def _by_walker(E_slot, walker):
    """History rows by slot -> by walker."""
    out = np.empty_like(E_slot)
    np.put_along_axis(out, walker.astype(np.int64), E_slot, axis=-1)
    return out


# ---------------------------------------------------------------- a walker is the single handle
_WALKER_CASES = [("one", 1, 1), ("one", 3, 1), ("chain7", 3, 1), ("chain7", 17, 1), ("g200", 1, 1), ("g200", 3, 1), ("g200", 17, 2),
                 ("g200", 65, 1), ("g5000", 3, 1), ("g5000", 17, 1), ("g5000", 65, 1), ("g40000", 1, 1), ("g40000", 3, 1), ("g40000", 17, 1),
                 ("g40000", 65, 1)]


# (n = 40000 is above K5S_MAX: the colour route only)
@pytest.mark.parametrize("route,name,R,ladders", [(r,) + c for c in _WALKER_CASES for r in ROUTES if not (r == "small" and c[0] == "g40000")])
def test_every_walker_is_the_single_handle_and_the_oracle(monkeypatch, route, name, R, ladders):
    """Swaps off, distinct temperatures, 3 sweeps: walker g == SparseSystem.sweep(T_w, 3, seed, 0, replica=g) == the oracle, from the
    contract's random start."""
    from tsu import _hip
    from tsu.models import GraphTempering
    A, bias = _graph(name)
    n = A.shape[0]
    _route(monkeypatch, route, n)
    temps = np.linspace(0.6, 3.0, R) if R > 1 else np.array([0.9])
    seed = 1234 + R
    with GraphTempering(A, temps, bias=bias, ladders=ladders, seed=seed) as pt:
        assert pt.plan()["route"] == route
        start = [pt.state(w, ladder=k) for k in range(ladders) for w in range(R)]
        for g, s in enumerate(start):
            np.testing.assert_array_equal(s, twin.random_start(n, g, seed), err_msg=f"random start of walker {g}")
        pt.run(1, 3, swap=False, record=False)
        assert pt.sweep_count == 3
        got = [pt.state(w, ladder=k) for k in range(ladders) for w in range(R)]
        single = _hip.SparseSystem(A.indptr, A.indices, A.data, bias, pt.color_offsets, pt.order)
        for g in range(R * ladders):
            T = float(temps[g % R])
            want = ora.sparse_sweep_philox(start[g], A.indptr, A.indices, A.data, bias, T, 3, seed, sweep0=0, replica=g, order=pt.order)
            np.testing.assert_array_equal(got[g], want, err_msg=f"walker {g} against the oracle")
            if g < 20 or g == R * ladders - 1:  # the handle-by-handle route: the first walkers and the last
                single.set_state(start[g])
                single.sweep(T, 3, seed=seed, sweep0=0, replica=g)
                np.testing.assert_array_equal(got[g], single.get_state(), err_msg=f"walker {g} against SparseSystem")
        single.close()


# ---------------------------------------------------------------- a tempering run is the twin
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("kind", ["gaussian", "dyadic"])
def test_a_tempering_run_is_the_twin(monkeypatch, route, kind):
    """n = 64, 5 temperatures, 2 ladders, 20 rounds of 3 sweeps: history, counters, tables and final states.  Gaussian couplings: the twin
    is fed the device's energies; dyadic couplings: it uses its own."""
    from tsu.models import GraphTempering
    A, bias = _graph("g64") if kind == "gaussian" else _dyadic(64, 9)
    _route(monkeypatch, route, 64)
    temps = [0.7, 1.0, 1.4, 2.0, 2.9]
    with GraphTempering(A, temps, bias=bias, ladders=2, seed=42) as pt:
        pt.run(20, 3)
        hist = [pt.history(ladder=k) for k in range(2)]
        E = np.stack([h["E"] for h in hist], axis=1)
        M = np.stack([h["M"] for h in hist], axis=1)
        W = np.stack([h["walker"] for h in hist], axis=1)
        E_walker = _by_walker(E, W)
        b = twin.Batch(A, bias, pt.order, temps, ladders=2, seed=42)
        tE, tM, tW = b.run(20, 3, energies=(lambda j, _b: E_walker[j].reshape(-1)) if kind == "gaussian" else None)
        np.testing.assert_array_equal(W, tW)
        np.testing.assert_array_equal(M, tM)
        np.testing.assert_array_equal(E, tE)
        attempts, accepts = pt.swap_counts()
        np.testing.assert_array_equal(attempts, b.attempts)
        np.testing.assert_array_equal(accepts, b.accepts)
        assert attempts.sum() == 2 * 4 * 20 and 0 < accepts.sum() < attempts.sum()
        np.testing.assert_array_equal(pt.round_trips(), b.trips)
        np.testing.assert_array_equal(pt.walker_at_slot(), b.walker_at_slot)
        assert pt.sweep_count == 60 == b.sweeps
        for k in range(2):
            for i in range(5):
                np.testing.assert_array_equal(pt.state(i, ladder=k), b.state_at(i, ladder=k))
        acc = pt.acceptance()
        np.testing.assert_allclose(acc, b.accepts / b.attempts)


# ---------------------------------------------------------------- energies
@pytest.mark.parametrize("name", ["g200", "g5000", "g70000"])
def test_energies_are_fixed_order_sums(monkeypatch, name):
    """Gaussian couplings: the same bits on two runs, on both routes (n <= 32768) and in the twin's fixed-order function; n = 70000 has
    two energy segments."""
    from tsu.models import GraphTempering
    A, bias = _graph(name)
    n = A.shape[0]
    seen = []
    for route in ROUTES:
        if route == "small" and n > K5S_MAX:
            continue
        if route == "colour":
            monkeypatch.setenv("TSU_K5B_SMALL", "0")
        else:
            monkeypatch.delenv("TSU_K5B_SMALL", raising=False)
        for _ in range(2):
            with GraphTempering(A, [0.8, 1.1, 1.5, 2.0, 2.7], bias=bias, seed=5) as pt:
                pt.run(2, 2, swap=False)
                E = pt.history()["E"]
                now = pt.energies()[0]
                np.testing.assert_array_equal(E[-1], now)  # run's pass (small route: inside k5b_small) == the colour route's passes
                seen.append(E)
                states = [pt.state(i) for i in range(5)]
                order = pt.order
    for E in seen[1:]:
        np.testing.assert_array_equal(E, seen[0])
    want = [twin.fixed_order_energy(s, A, bias, order) for s in states]
    np.testing.assert_array_equal(seen[0][-1], want)
    for s, e in zip(states, want):
        assert e == pytest.approx(ora.sparse_energy(s, A.indptr, A.indices, A.data, bias), rel=1e-12)


@pytest.mark.parametrize("route", ROUTES)
def test_energies_are_exact_on_dyadic_couplings(monkeypatch, route):
    from tsu.models import GraphTempering
    A, bias = _dyadic(300, 3)
    _route(monkeypatch, route, 300)
    with GraphTempering(A, [0.5, 0.8, 1.3], bias=bias, ladders=3, seed=8) as pt:
        pt.run(3, 2)
        E = pt.energies()
        M = [h["M"][-1] for h in (pt.history(ladder=k) for k in range(3))]
        for k in range(3):
            for i in range(3):
                s = pt.state(i, ladder=k)
                assert E[k, i] == ora.sparse_energy(s, A.indptr, A.indices, A.data, bias)
                assert pt.energy(i, ladder=k) == E[k, i]
                assert M[k][i] == int((2 * s.astype(int) - 1).sum())


# ---------------------------------------------------------------- best states
@pytest.mark.parametrize("route", ROUTES)
def test_best_states_are_the_twins(monkeypatch, route):
    """Dyadic couplings (the twin's own energies are the device's): the best state and energy equal the twin's, the energy is the
    energy of the returned bits; with tracking off the launch count and every result of the run are what they are without it."""
    from tsu.models import GraphTempering
    A, bias = _dyadic(64, 11)
    _route(monkeypatch, route, 64)
    temps = [0.4, 0.7, 1.2, 2.0]
    res = {}
    for track in (False, True):
        with GraphTempering(A, temps, bias=bias, ladders=2, seed=21, track_best=track) as pt:
            pt.run(12, 2)
            h = pt.history()
            res[track] = (h["E"], h["M"], h["walker"], pt.walker_at_slot(), [pt.state(i, ladder=1) for i in range(4)], pt.launch_count)
            if track:
                bits, e = pt.best()
                b = twin.Batch(A, bias, pt.order, temps, ladders=2, seed=21, track_best=True)
                b.run(12, 2)
                tbits, te = b.best()
                assert e == te
                np.testing.assert_array_equal(bits, tbits)
                assert e == ora.sparse_energy(bits, A.indptr, A.indices, A.data, bias)
                assert e <= h["E"].min()
            else:
                with pytest.raises(ValueError, match="track_best"):
                    pt.best()
    for a, b_ in zip(res[False][:5], res[True][:5]):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b_))
    per_round = 2 if route == "small" else 2 * pt.n_colors + 3
    assert res[False][5] == 12 * per_round                  # tracking off: the launches of a run without it
    assert res[True][5] == 12 * (per_round + 2) + 4         # on: two small launches per round, and the start's candidates once


def test_the_initial_state_is_a_candidate():
    """All-ones start at a high temperature on a ferromagnetic ring with a field: nothing the run visits is lower than the start."""
    from tsu.graph import canonical_csr
    from tsu.models import GraphTempering
    n = 32
    ring = sp.diags([np.ones(n - 1), np.ones(n - 1), [1.0], [1.0]], [1, -1, n - 1, -(n - 1)])
    A = canonical_csr(ring)
    bias = np.full(n, 0.5)
    with GraphTempering(A, [50.0, 60.0], bias=bias, seed=3, initial="ones", track_best=True) as pt:
        pt.run(3, 1, swap=False)
        bits, e = pt.best()
        np.testing.assert_array_equal(bits, np.ones(n, np.int8))
        assert e == ora.sparse_energy(bits, A.indptr, A.indices, A.data, bias) == -1.5 * n


# ---------------------------------------------------------------- anneal
@pytest.mark.parametrize("route", ROUTES)
def test_anneal_is_the_twin_and_the_stream_continues(monkeypatch, route):
    from tsu.models import GraphTempering
    A, bias = _dyadic(64, 13)
    _route(monkeypatch, route, 64)
    temps = [1.0, 1.0, 1.0]
    rows = np.array([[3.0, 2.5, 2.0], [2.0, 1.8, 1.5], [1.2, 1.0, 0.9], [0.6, 0.5, 0.4]])
    with GraphTempering(A, temps, bias=bias, ladders=2, seed=17, track_best=True) as pt:
        b = twin.Batch(A, bias, pt.order, temps, ladders=2, seed=17, track_best=True)
        pt.anneal([4.0, 3.0], sweeps_per_step=2)       # one temperature per step for every walker
        pt.anneal(rows, sweeps_per_step=2)              # a row per step: 6 steps in all
        b.anneal([4.0, 3.0], 2)
        b.anneal(rows, 2)
        assert pt.sweep_count == 12 == b.sweeps
        for k in range(2):
            for i in range(3):
                np.testing.assert_array_equal(pt.state(i, ladder=k), b.state_at(i, ladder=k))
        bits, e = pt.best()
        tbits, te = b.best()
        assert e == te
        np.testing.assert_array_equal(bits, tbits)
        pt.run(4, 2)                                    # the sweep counter, the stream and the last temperatures go on
        tE, tM, tW = b.run(4, 2)
        h = [pt.history(ladder=k) for k in range(2)]
        np.testing.assert_array_equal(np.stack([x["walker"] for x in h], axis=1), tW)
        np.testing.assert_array_equal(np.stack([x["E"] for x in h], axis=1), tE)
        np.testing.assert_array_equal(np.stack([x["M"] for x in h], axis=1), tM)
        assert pt.sweep_count == 20
        with pytest.raises(ValueError, match="Temperature must be positive"):
            pt.anneal([1.0, 0.0])
        with pytest.raises(ValueError, match="shape"):
            pt.anneal(np.ones((2, 2)))


# ---------------------------------------------------------------- launches
@pytest.mark.parametrize("route", ROUTES)
def test_plan_and_launch_counts(monkeypatch, route):
    from tsu.models import GraphTempering
    A, bias = _graph("g200")
    _route(monkeypatch, route, 200)
    with GraphTempering(A, [0.8, 1.0, 1.3, 1.7, 2.2, 3.0], bias=bias, seed=2) as pt:
        p = pt.plan()
        assert p["route"] == route and p["padded_walkers"] == 16 and p["energy_segments"] == 1
        assert pt.launch_count == 0
        pt.run(5, 4)
        if route == "small":
            assert p["walkers_per_thread"] == 1 and p["launches_per_sweep"] == 0 and p["launches_per_round_fixed"] == 2
            assert pt.launch_count == 5 * 2                           # the round's sweeps and energies, then the swap pass
        else:
            assert p["walkers_per_thread"] == 8 and p["launches_per_sweep"] == pt.n_colors and p["launches_per_round_fixed"] == 3
            assert pt.launch_count == 5 * (pt.n_colors * 4 + 2 + 1)   # a launch per colour class and sweep, two energy passes, the swap pass
        before = pt.launch_count
        pt.run(3, 4, swap=False, record=False)                        # nothing asks for energies or the swap pass
        assert pt.launch_count - before == 3 * (1 if route == "small" else pt.n_colors * 4)
    with GraphTempering(A, np.linspace(1.0, 2.0, 20), bias=bias, ladders=2) as pt:
        p = pt.plan()
        assert p["padded_walkers"] == 48 and p["walkers_per_thread"] == (1 if route == "small" else 8)
    if route == "colour":  # the chunk width changes the thread shape, not the results
        res = {}
        for chunk in ("", "4", "16"):
            if chunk:
                monkeypatch.setenv("TSU_K5B_CHUNK", chunk)
            with GraphTempering(A, np.linspace(1.0, 2.0, 20), bias=bias, seed=6) as pt:
                assert pt.plan()["walkers_per_thread"] == int(chunk or 8)
                pt.run(2, 2)
                res[chunk] = ([pt.state(i) for i in range(20)], pt.history()["E"])
        for chunk in ("4", "16"):
            np.testing.assert_array_equal(res[chunk][0], res[""][0])
            np.testing.assert_array_equal(res[chunk][1], res[""][1])


def test_c_abi_checks_its_arguments():
    from tsu import _hip
    A, bias = _graph("chain7")
    from tsu.graph import color_graph
    off, order = color_graph(A)
    g = _hip.SparseSystem(A.indptr, A.indices, A.data, bias, off, order)
    for R, nl, msg in ((0, 1, "n_temps"), (257, 1, "n_temps"), (2, 0, "n_ladders"), (256, 256, "65535 walkers")):
        with pytest.raises(ValueError, match="tsu_sparse_batch_create: .*" + msg):
            _hip.SparseBatch(g, R, nl)
    b = _hip.SparseBatch(g, 2, 1)
    with pytest.raises(ValueError, match="tsu_sparse_batch_run: call tsu_sparse_batch_set_temperatures first"):
        b.run(1, 1)
    with pytest.raises(ValueError, match="Temperature must be positive"):
        b.set_temperatures([1.0, 0.0])
    b.set_temperatures([1.0, 2.0])
    with pytest.raises(ValueError, match="tsu_sparse_batch_run: call tsu_sparse_batch_init first"):
        b.run(1, 1)
    with pytest.raises(ValueError, match="tsu_sparse_batch_init: initial"):
        b.init(1, 2)
    b.init(1, 0)
    with pytest.raises(ValueError, match="tsu_sparse_batch_run: need"):
        b.run(1, 0)
    with pytest.raises(ValueError, match="tsu_sparse_batch_get_state: ladder 0, slot 2 out of range"):
        b.get_state(0, 2)
    with pytest.raises(ValueError, match="state must be 0/1"):
        b.set_state(0, 0, np.full(7, 2, np.int8))
    with pytest.raises(ValueError, match="tsu_sparse_batch_best: call tsu_sparse_batch_track_best first"):
        b.best(0)
    st = np.array([1, 0, 1, 1, 0, 0, 1], np.int8)
    b.set_state(0, 1, st)
    np.testing.assert_array_equal(b.get_state(0, 1), st)
    b.close()
    g.close()


# ---------------------------------------------------------------- GibbsSampler.parallel_tempering on a sparse graph
def test_parallel_tempering_takes_a_sparse_coupling():
    from tsu.gibbs import GibbsConfig, GibbsSampler
    n = 30
    A = random_graph(n, 0.1, 30)
    bias = np.random.default_rng(30).normal(size=n)
    temps = [0.8, 1.2, 1.8, 2.7]

    def call(coupling):
        np.random.seed(123)
        s = GibbsSampler(GibbsConfig(temperature=1.0, n_burnin=5, n_sweeps=2), seed=99)
        return s.parallel_tempering(coupling, temps, bias, n_samples=25, swap_interval=4)

    samples, info = call(A)
    again, info2 = call(A)
    dense_samples, dense_info = call(A.toarray())
    assert samples.shape == dense_samples.shape == (25, n) and samples.dtype == dense_samples.dtype
    assert set(np.unique(samples)) <= {0, 1}
    assert set(info) == set(dense_info)
    np.testing.assert_array_equal(samples, again)
    assert info["energies"] == info2["energies"]
    assert info["swap_attempts"] == (25 // 4) * (len(temps) - 1) == dense_info["swap_attempts"]
    assert 0 <= info["swap_accepts"] <= info["swap_attempts"]
    assert info["swap_acceptance_rate"] == info["swap_accepts"] / info["swap_attempts"]
    assert len(info["energies"]) == len(temps) and all(len(e) == 25 for e in info["energies"])
    assert len(info["final_states"]) == len(temps) and all(np.asarray(s).shape == (n,) for s in info["final_states"])
    np.testing.assert_array_equal(samples[-1], info["final_states"][0])
    for i, s in enumerate(info["final_states"]):
        assert info["energies"][i][-1] == pytest.approx(ora.sparse_energy(np.asarray(s, np.int8), A.indptr, A.indices, A.data, bias), rel=1e-12)
    # dense input takes the dense path as before: reproducible, and different draws from the sparse branch's
    dense_again, _ = call(A.toarray())
    np.testing.assert_array_equal(dense_samples, dense_again)
    assert len(dense_info["energies"][0]) == 25

"""Tempering ladders of 65 to 256 temperatures on the GPU (-m gpu): the one-wave swap pass k7_pt_swap (csrc/pt_dev.h) past its first
trip of 64 lanes, the per-slot passes (overlap, link overlap, profiles, modes, cluster moves) at slots >= 64, the walker-group loop of
the sweeps over hundreds of walkers, and the sparse walker batches with swaps.

Everything is compared with the NumPy twins run on their OWN energies from the start the helper computes (tests/helpers/
long_ladder.py: dyadic disorder, so the device's fixed-order sums equal the twins' float64 energies with ==): nothing of the device
feeds the reference.  tests/test_long_ladders_cpu.py asserts, from the twins alone, that these runs accept and refuse swaps of pairs
past lane 63, move walkers through the slots >= 64 and flip clusters there.

  A  whole runs with swaps, 2-D and 3-D raw handles, R = 64 .. 256, the automatic walker group and TSU_PT_GROUP = 7 / nl R
  B  the conveyor: with equal energies every pair is accepted, and 2 R + 3 rounds give every walker round trips in a closed form
  C  q, q_link and the k_min modes of every slot of a 130-temperature pair of ladders, every round
  D  cluster moves over a slot list of 100 of 130 slots, both routes
  F  GraphTempering with swaps, R = 65 and 256, both routes
(E, the ensembles, is in tests/test_ensemble_gpu.py.)"""
import importlib.util
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _helper():
    """One instance per process, so that the CPU and the GPU file share the twins' runs when both are collected."""
    name = "tsu_tests_long_ladder"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "helpers", "long_ladder.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


ll = _helper()


@pytest.fixture(scope="module")
def hip():
    from tsu import _hip
    return _hip


def _handle(hip, shape, periodic, R, ladders, dis, seed=ll.LADDER_SEED):
    """The raw handle on `dis`, temperatures(R), random start."""
    cls = hip.TemperingLattice if len(shape) == 2 else hip.TemperingLattice3D
    pt = cls(*shape, periodic, R, ladders)
    try:
        pt.set_disorder(*dis)
        pt.set_temperatures(ll.temperatures(R))
        return pt
    except BaseException:
        pt.close()
        raise


def _group(monkeypatch, group, nw):
    if group == "auto":
        monkeypatch.delenv("TSU_PT_GROUP", raising=False)
    else:
        monkeypatch.setenv("TSU_PT_GROUP", str(nw) if group == "nlR" else group)


def _same_tables(st, want, what):
    for key in ("attempts", "accepts", "round_trips", "walker_at_slot"):
        assert np.array_equal(st[key], want[key]), f"{what}: {key} differs at {np.argwhere(st[key] != want[key])[:8].tolist()}"
    assert st["sweep_count"] == want["sweep_count"] and st["round_count"] == want["round_count"], what


# ---------------------------------------------------------------- A. whole runs with swaps
_A_CASES = [c + ("auto",) for c in ll.LATTICE_CASES] + [c + (g,) for c in (ll.LATTICE_CASES[0], ll.LATTICE_CASES[4]) for g in ("7", "nlR")]


@pytest.mark.parametrize("shape,periodic,ladders,R,group", _A_CASES)
def test_whole_runs_equal_the_twin(hip, monkeypatch, shape, periodic, ladders, R, group):
    """run(4, 2) then run(3, 1), swapping and recording: after each the history (walker, M, E with ==, q), the tables and the
    counters equal the twin's; at the end every slot's spins and every walker's energy do.  The twin starts from the helper's start
    and runs on its own energies."""
    _group(monkeypatch, group, ladders * R)
    want = ll.lattice_run(shape, periodic, ladders, R)
    pt = _handle(hip, shape, periodic, R, ladders, want["dis"])
    try:
        pt.init(ll.LADDER_SEED, 0)
        for (n, interval), (hist_w, tables_w) in zip(ll.RUNS, want["after"]):
            pt.run(n, interval, swap=True, record=True)
            hist = pt.history()
            what = f"{shape} R={R} group {group} after run({n}, {interval})"
            for key in ("walker", "M", "E"):
                assert np.array_equal(hist[key], hist_w[key]), f"{what}: {key} differs at {np.argwhere(hist[key] != hist_w[key])[:8].tolist()}"
            if ladders == 2:
                assert np.array_equal(hist["q"], hist_w["q"]), f"{what}: q"
            else:
                assert hist["q"] is None
            _same_tables(pt.stats(), tables_w, what)
        E, M = pt.energies()
        assert np.array_equal(E, want["E"]), np.argwhere(E != want["E"])[:8].tolist()
        was = want["after"][-1][1]["walker_at_slot"]
        for k in range(ladders):
            for i in range(R):
                s = want["spins"][k][was[k, i]]
                got = pt.get_spins(k, i)
                assert np.array_equal(got, s), f"ladder {k} slot {i}: {int((got != s).sum())} sites differ"
                assert M[k, was[k, i]] == int(s.sum(dtype=np.int64))
    finally:
        pt.close()


# ---------------------------------------------------------------- B. the conveyor
def _assert_conveyor(R, n, ladders, rows, st, what):
    want = ll.conveyor(R, n)
    for k in range(ladders):
        assert np.array_equal(rows[:, k], want["rows"]), f"{what}: recorded walker rows of ladder {k}"
        assert np.array_equal(st["walker_at_slot"][k], want["walker_at_slot"]), f"{what}: walker_at_slot of ladder {k}"
        assert (st["attempts"][k] == n).all() and (st["accepts"][k] == n).all(), f"{what}: attempts / accepts of ladder {k}"
        assert np.array_equal(st["round_trips"][k], want["round_trips"]), (what, k, st["round_trips"][k].tolist())


@pytest.mark.parametrize("shape,periodic", [((4, 8), True), ((2, 4, 8), (False, True, True))])
@pytest.mark.parametrize("R", [65, 256])
@pytest.mark.parametrize("ladders", [1, 2])
def test_conveyor(hip, monkeypatch, shape, periodic, R, ladders):
    """All couplings 0 and no field (the handles take that): every energy is 0, every delta +-0, every pair accepted.  After
    n = 2 R + 3 rounds of one sweep walker_at_slot[i] = (i + n) % R, accepts = attempts = n and round_trips[w] = (n - w) // R: round
    trips of walkers past lane 63, which no short random run produces; the recorded walker rows are the rotation round by round."""
    monkeypatch.delenv("TSU_PT_GROUP", raising=False)
    n = 2 * R + 3
    pt = _handle(hip, shape, periodic, R, ladders, ll.zero_disorder(shape))
    try:
        pt.init(ll.LADDER_SEED, 0)
        pt.run(n, 1, swap=True, record=True)
        hist = pt.history()
        assert (hist["E"] == 0).all()
        _assert_conveyor(R, n, ladders, hist["walker"], pt.stats(), f"{shape} R={R}")
        assert pt.stats()["sweep_count"] == n
    finally:
        pt.close()


def test_conveyor_of_a_sparse_batch(hip):
    """The same through SparseBatch (its own tables, the shared swap pass): the chain of 7 sites with couplings and bias 0."""
    from tsu.graph import color_graph
    from test_sparse_batch_gpu import _graph  # (tests/ is on sys.path: rootdir conftest, prepend import mode)
    R, ladders = 256, 2
    n = 2 * R + 3
    A = _graph("chain7")[0].copy()
    A.data[:] = 0.0  # the chain's pattern with explicit zeros
    assert A.nnz == 12
    off, order = color_graph(A)
    g = hip.SparseSystem(A.indptr, A.indices, A.data, np.zeros(7), off, order)
    b = hip.SparseBatch(g, R, ladders)
    try:
        b.set_temperatures(ll.temperatures(R))
        b.init(ll.LADDER_SEED, 0)
        b.run(n, 1)
        E, M, W = b.history()
        assert (E == 0).all()
        _assert_conveyor(R, n, ladders, W, b.stats(), "chain7")
    finally:
        b.close()
        g.close()


# ---------------------------------------------------------------- C. per-slot passes
def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.complex128, what
    assert not np.isnan(want.view(np.float64)).any()
    bad = np.argwhere(got.view(np.float64).view(np.uint64) != want.view(np.float64).view(np.uint64))
    assert bad.size == 0, f"{what}: modes differ at {bad[:8].tolist()}"


@pytest.mark.parametrize("shape,periodic,ladders,R", ll.SLOT_PASS_CASES)
def test_per_slot_passes(hip, monkeypatch, shape, periodic, ladders, R):
    """Correlation and link overlap on, run(3, 2): for every round and slot q and q_link equal the twins' of the twin's planes at
    that slot with ==, the modes bit for bit; the values at the slots >= 64 are not all one value (no stuck row)."""
    monkeypatch.delenv("TSU_PT_GROUP", raising=False)
    want = ll.slot_pass_run(shape, periodic, ladders, R)
    pt = _handle(hip, shape, periodic, R, ladders, want["dis"])
    try:
        pt.set_correlation(True, [ll.correlation_twin.tables(n) if p else None for n, p in zip(shape, ll.axes(shape, periodic))])
        pt.set_link_overlap(True)
        pt.init(ll.LADDER_SEED, 0)
        pt.run(3, 2, swap=True, record=True)
        hist = pt.history()
        modes = pt.history_modes()
        assert np.array_equal(hist["walker"], want["walker"])
        for key in ("q", "q_link"):
            assert hist[key].dtype == np.int64
            assert np.array_equal(hist[key], want[key]), f"{key} differs at {np.argwhere(hist[key] != want[key])[:8].tolist()}"
            assert all(len(np.unique(hist[key][j, 64:])) > 1 for j in range(3)), key
        _same_bits(modes, want["modes"], f"{shape}")
        assert all(len(np.unique(modes[j, 64:])) > 1 for j in range(3))
        _same_tables(pt.stats(), want["tables"], f"{shape}")
    finally:
        pt.close()


# ---------------------------------------------------------------- D. cluster moves over a long slot list
@pytest.mark.parametrize("edge", [None, "8"])
def test_cluster_moves_over_100_slots(hip, monkeypatch, edge):
    """(12, 16) periodic, two ladders of 130, cluster moves every round over the 100 slots below t_max, on the one-launch route and
    the tiled one: three rounds against icm_twin.Ladders on its own energies; the slots >= 100 flip nothing, some slot in [64, 100)
    does."""
    monkeypatch.delenv("TSU_PT_GROUP", raising=False)
    if edge is None:
        monkeypatch.delenv("TSU_ICM_TILE", raising=False)
    else:
        monkeypatch.setenv("TSU_ICM_TILE", edge)
    want = ll.icm_run()
    R, n_in = ll.ICM_R, ll.ICM_SLOTS
    pt = _handle(hip, ll.ICM_SHAPE, True, R, 2, want["dis"])
    try:
        pt.set_cluster_moves(1, ll.icm_t_max())
        pt.init(ll.LADDER_SEED)
        pt.run(3, 2, swap=True, record=True)
        hist = pt.history()
        for key in ("walker", "M", "E", "q"):
            assert np.array_equal(hist[key], want["hist"][key]), f"{key} differs at {np.argwhere(hist[key] != want['hist'][key])[:8].tolist()}"
        _same_tables(pt.stats(), want["tables"], f"edge {edge}")
        E, _ = pt.energies()
        assert np.array_equal(E, want["E"])
        was = want["tables"]["walker_at_slot"]
        for k in range(2):
            for i in range(R):
                assert np.array_equal(pt.get_spins(k, i), want["spins"][k][was[k, i]]), (k, i)
        cs = pt.cluster_stats()
        assert cs["pass_count"] == want["passes"] == 3 and np.array_equal(cs["passes"], want["slot_passes"])
        assert np.array_equal(cs["clusters"], want["clusters"]) and np.array_equal(cs["flipped"], want["flipped"])
        assert (cs["flipped"][n_in:] == 0).all() and (cs["clusters"][n_in:] == 0).all() and (cs["passes"][n_in:] == 0).all()
        assert (cs["flipped"][64:n_in] > 0).any()
        assert cs["launches"] == (9 if edge else 3)
    finally:
        pt.close()


# ---------------------------------------------------------------- F. sparse batches with swaps
@pytest.mark.parametrize("route", ["small", "colour"])
@pytest.mark.parametrize("R", [65, 256])
def test_a_long_sparse_tempering_run_is_the_twin(hip, monkeypatch, route, R):
    """test_sparse_batch_gpu.test_a_tempering_run_is_the_twin with 65 and 256 temperatures (helper: sparse_temperatures), two ladders,
    6 rounds of 2 sweeps on _dyadic(64, 9); the twin uses its own energies."""
    from tsu.models import GraphTempering
    from test_sparse_batch_gpu import _dyadic  # (tests/ is on sys.path: rootdir conftest, prepend import mode)
    A, bias = _dyadic(64, 9)
    if route == "colour":
        monkeypatch.setenv("TSU_K5B_SMALL", "0")
    else:
        monkeypatch.delenv("TSU_K5B_SMALL", raising=False)
    tE, tM, tW, b = ll.sparse_run(R)
    n, k = ll.SPARSE_ROUNDS, ll.SPARSE_INTERVAL
    with GraphTempering(A, ll.sparse_temperatures(R), bias=bias, ladders=2, seed=ll.SPARSE_SEED) as pt:
        assert pt.plan()["route"] == route and np.array_equal(pt.order, b.order)
        pt.run(n, k)
        hist = [pt.history(ladder=j) for j in range(2)]
        np.testing.assert_array_equal(np.stack([h["walker"] for h in hist], axis=1), tW)
        np.testing.assert_array_equal(np.stack([h["M"] for h in hist], axis=1), tM)
        np.testing.assert_array_equal(np.stack([h["E"] for h in hist], axis=1), tE)
        attempts, accepts = pt.swap_counts()
        np.testing.assert_array_equal(attempts, b.attempts)
        np.testing.assert_array_equal(accepts, b.accepts)
        assert attempts.sum() == 2 * (R - 1) * n and 0 < accepts.sum() < attempts.sum()
        np.testing.assert_array_equal(pt.round_trips(), b.trips)
        np.testing.assert_array_equal(pt.walker_at_slot(), b.walker_at_slot)
        assert pt.sweep_count == n * k == b.sweeps
        for j in range(2):
            for i in range(R):
                np.testing.assert_array_equal(pt.state(i, ladder=j), b.state_at(i, ladder=j))
        np.testing.assert_allclose(pt.acceptance(), b.accepts / b.attempts)

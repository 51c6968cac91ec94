"""Tempering ladders of 65 to 256 temperatures, without a device (tests/helpers/long_ladder.py): the dyadic energies do not depend on
the order of summation, the conveyor's closed form is tempering_twin.swap_pass with equal energies, and the twins' runs that
tests/test_long_ladders_gpu.py compares the device with do reach what they are there for -- accepted AND refused swaps of pairs past
lane 63 of the one-wave swap pass, slots >= 64 that change hands, cluster moves that flip sites at slots >= 64.  These are conditions
on the cases, asserted from the twins alone, so a pass on the GPU cannot be vacuous."""
import importlib.util
import os
import sys

import numpy as np
import pytest

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


# ---------------------------------------------------------------- the helper
@pytest.mark.parametrize("shape,periodic", [((6, 10), True), ((5, 37), False), ((3, 5, 9), False), ((3, 4, 16), (False, True, True))])
def test_dyadic_energies_do_not_depend_on_the_order(shape, periodic):
    dis = ll.dyadic_disorder(shape, periodic, ll.DISORDER_SEED)
    per = ll.axes(shape, periodic)
    nd = len(shape)
    for j, J in enumerate(dis[:nd]):
        assert J.dtype == np.float32 and (J * 8 == np.rint(J * 8)).all() and np.abs(J).max() <= 1.0
        if not per[nd - 1 - j]:
            assert (np.take(J, -1, axis=nd - 1 - j) == 0).all()
        assert len(np.unique(J)) > 8
    assert (dis[nd] * 8 == np.rint(dis[nd] * 8)).all() and np.abs(dis[nd]).max() <= 0.5
    rng = np.random.default_rng(1)
    for s in ll.start(shape, 5, 3):
        terms = ll.energy_terms(s, periodic, dis)
        forward = 0.0
        for t in terms:
            forward += t
        backward = 0.0
        for t in rng.permutation(terms)[::-1]:
            backward += t
        assert forward == backward == np.sum(terms) == np.sum(terms.astype(np.float32), dtype=np.float32)
        assert -forward == ll.energy(s, periodic, dis)


def test_start_is_the_ladders_random_start():
    a = ll.start((6, 10), 77, 4)
    b = ll.tempering3d_twin.initial_spins((1, 6, 10), 77, 4)
    assert a.shape == (4, 6, 10) and a.dtype == np.int8
    assert all((a[g] == b[g].reshape(6, 10)).all() for g in range(4))
    assert (ll.temperatures(130) == np.geomspace(0.3, 4.0, 130)).all()
    T = ll.temperatures(ll.ICM_R)
    assert T[ll.ICM_SLOTS - 1] < ll.icm_t_max() < T[ll.ICM_SLOTS]


# ---------------------------------------------------------------- B. the conveyor
@pytest.mark.parametrize("R", [2, 3, 65, 256])
def test_conveyor_is_the_swap_pass_with_equal_energies(R):
    n = 2 * R + 3
    want = ll.conveyor(R, n)
    for splits in ((n,), (R + 1, n - R - 1)):
        got = ll.conveyor_rehearsal(R, splits)
        for key in ("walker_at_slot", "round_trips", "accepts", "rows"):
            assert np.array_equal(got[key], want[key]), (key, splits)
        assert (got["attempts"] == n).all()
    if R >= 65:  # round trips of walkers past lane 63, and of different counts
        assert want["round_trips"][64] >= 1 and len(set(want["round_trips"])) == 2


# ---------------------------------------------------------------- A. whole runs
@pytest.mark.parametrize("shape,periodic,ladders,R", ll.LATTICE_CASES)
def test_lattice_runs_swap_past_lane_63(shape, periodic, ladders, R):
    run = ll.lattice_run(shape, periodic, ladders, R)
    tables = run["after"][-1][1]
    assert tables["round_count"] == 7 and tables["sweep_count"] == 11
    assert (tables["attempts"] == 7).all()
    cov = ll.coverage(tables["attempts"], tables["accepts"], tables["walker_at_slot"])
    print(shape, R, cov)
    if R >= 129:
        for high, low, moved in cov:
            assert high >= 8 and low >= 8 and moved >= 0.5, cov
    elif R == 65:
        rows = np.concatenate([h["walker"] for h, _ in run["after"]])
        assert (rows[:, :, 64] != 64).any(), "slot 64 never changed hands"
    assert tables["accepts"].sum() > 0
    for k in range(ladders):
        assert sorted(tables["walker_at_slot"][k]) == list(range(R))


# ---------------------------------------------------------------- C. per-slot passes
@pytest.mark.parametrize("shape,periodic,ladders,R", ll.SLOT_PASS_CASES)
def test_slot_pass_rows_differ_past_slot_63(shape, periodic, ladders, R):
    run = ll.slot_pass_run(shape, periodic, ladders, R)
    assert run["q"].shape == run["q_link"].shape == (3, R) and run["modes"].shape == (3, R, sum(ll.axes(shape, periodic)))
    for key in ("q", "q_link", "modes"):
        for j in range(3):
            assert len(np.unique(run[key][j, 64:])) > 8, key
    assert (run["walker"][-1][:, 64:] != np.arange(64, R)).any()


# ---------------------------------------------------------------- D. cluster moves
def test_cluster_moves_flip_sites_past_slot_63():
    run = ll.icm_run()
    assert run["passes"] == 3
    assert (run["slot_passes"][:ll.ICM_SLOTS] == 3).all() and (run["slot_passes"][ll.ICM_SLOTS:] == 0).all()
    assert (run["flipped"][ll.ICM_SLOTS:] == 0).all() and (run["clusters"][ll.ICM_SLOTS:] == 0).all()
    assert (run["flipped"][64:ll.ICM_SLOTS] > 0).any()
    assert (run["flipped"][64:ll.ICM_SLOTS] > 0).sum() >= 8, run["flipped"]
    assert run["tables"]["accepts"][:, 64:].sum() > 0


# ---------------------------------------------------------------- F. sparse batches
@pytest.mark.parametrize("R", [65, 256])
def test_sparse_runs_swap_past_lane_63(R):
    from test_sparse_batch_gpu import _dyadic  # (tests/ is on sys.path: rootdir conftest, prepend import mode)
    A, bias = _dyadic(64, 9)
    A2, bias2 = ll.sparse_dyadic(64, 9)
    assert (A != A2).nnz == 0 and np.array_equal(bias, bias2)
    E, M, W, b = ll.sparse_run(R)
    assert W.shape == (ll.SPARSE_ROUNDS, 2, R) and (b.attempts == ll.SPARSE_ROUNDS).all()
    cov = ll.coverage(b.attempts, b.accepts, b.walker_at_slot)
    print(R, cov)
    if R >= 129:
        for high, low, moved in cov:
            assert high >= 8 and low >= 8 and moved >= 0.5, cov
    else:
        assert (W[:, :, 64] != 64).any(), "slot 64 never changed hands"

"""K7 parallel tempering on the host: the NumPy twin's swap pass against a literal restatement of the reference's rule
(gibbs.py:309-323; its energy difference has the opposite sign) and against detailed balance, the round-trip bookkeeping, the swap uniforms against dense_uniform's construction, validation before the
device is touched, and the new C-ABI symbols (no GPU needed)."""
import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest

from oracle import oracle as ora

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_spec = importlib.util.spec_from_file_location("tempering_twin", os.path.join(HERE, "helpers", "tempering_twin.py"))
twin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(twin)

PT_SYMBOLS = ["tsu_pt2d_create", "tsu_pt2d_destroy", "tsu_pt2d_set_disorder", "tsu_pt2d_set_temperatures", "tsu_pt2d_init",
              "tsu_pt2d_run", "tsu_pt2d_history", "tsu_pt2d_stats", "tsu_pt2d_energies", "tsu_pt2d_get_spins", "tsu_pt2d_set_spins",
              "tsu_pt2d_launch_count"]


def _reference_pass(states, temperatures, compute_energy, rand):
    """gibbs.py:309-323 as written, with compute_energy(state) and the uniform of pair i as rand(i)."""
    n_replicas = len(temperatures)
    swap_attempts = swap_accepts = 0
    for i in range(n_replicas - 1):
        E_i = compute_energy(states[i])
        E_j = compute_energy(states[i + 1])
        T_i = temperatures[i]
        T_j = temperatures[i + 1]
        delta = (1.0 / T_i - 1.0 / T_j) * (E_j - E_i)
        swap_attempts += 1
        if delta >= 0 or rand(i) < np.exp(delta):
            states[i], states[i + 1] = states[i + 1], states[i]
            swap_accepts += 1
    return swap_attempts, swap_accepts


@pytest.mark.parametrize("trial", range(40))
def test_swap_pass_equals_reference_rule(trial):
    rng = np.random.default_rng(trial)
    R = int(rng.integers(2, 13))
    T = list(np.sort(rng.uniform(0.2, 4.0, R)))
    E = rng.normal(scale=float(rng.choice([0.1, 3.0, 50.0])), size=R)
    u = twin.swap_uniforms(R, int(rng.integers(0, 1000)), int(rng.integers(0, 2 ** 40)), int(trial & 1))
    states = list(range(R))  # a "state" is the walker's name
    # the reference's delta (E_j - E_i) is the detailed-balance ratio of -E: fed -E it makes the decisions of the lattice rule
    att, acc = _reference_pass(states, T, lambda s: -E[s], lambda i: u[i])
    was = np.arange(R)
    a, c = np.zeros(R - 1, np.int64), np.zeros(R - 1, np.int64)
    flags, trips = np.full(R, twin.NONE), np.zeros(R, np.int64)
    flags[0] = twin.BOTTOM
    twin.swap_pass(was, T, E, u, a, c, flags, trips)
    assert was.tolist() == states
    assert a.sum() == att == R - 1 and c.sum() == acc


def test_swap_rule_satisfies_detailed_balance():
    """Two slots, two walkers with energies Ea (slot 0) and Eb: P(swap) = min(1, w(after) / w(before)) for Boltzmann weights."""
    T = [0.5, 2.0]
    for Ea, Eb in ((-3.0, -1.0), (-1.0, -3.0), (2.0, 2.0)):
        before = math.exp(-Ea / T[0] - Eb / T[1])
        after = math.exp(-Eb / T[0] - Ea / T[1])
        p = min(1.0, after / before)
        for u in (0.0, 0.999999 * p, min(p * 1.000001, 0.9999999), 0.9999999):
            was = np.arange(2)
            a, c = np.zeros(1, np.int64), np.zeros(1, np.int64)
            twin.swap_pass(was, T, np.array([Ea, Eb]), np.array([u]), a, c, np.array([1, 0]), np.zeros(2, np.int64))
            assert bool(c[0]) == (u < p or p >= 1.0), (Ea, Eb, u, p)


def test_round_trip_bookkeeping_by_hand():
    # R = 3, every swap accepted (u = 0 < exp(delta) always): the pass moves the walker at slot 0 up to the last slot
    R, T, E = 3, [0.5, 1.0, 2.0], np.zeros(3)
    was = np.arange(R)
    a, c = np.zeros(R - 1, np.int64), np.zeros(R - 1, np.int64)
    flags, trips = np.full(R, twin.NONE), np.zeros(R, np.int64)
    flags[0] = twin.BOTTOM
    u = np.zeros(R - 1)
    # (walker at each slot, flag of each walker, round trips of each walker) after each pass
    expect = [([1, 2, 0], [twin.TOP, twin.BOTTOM, twin.NONE], [0, 0, 0]),
              ([2, 0, 1], [twin.TOP, twin.TOP, twin.BOTTOM], [0, 0, 0]),
              ([0, 1, 2], [twin.BOTTOM, twin.TOP, twin.TOP], [1, 0, 0])]
    for want_was, want_flags, want_trips in expect:
        twin.swap_pass(was, T, E, u, a, c, flags, trips)
        assert was.tolist() == want_was and flags.tolist() == want_flags and trips.tolist() == want_trips
    assert a.tolist() == [3, 3] and c.tolist() == [3, 3]
    # a walker that reaches the top without having been at the bottom does not start a round trip
    flags, trips = np.array([twin.NONE, twin.NONE]), np.zeros(2, np.int64)
    twin.arrive(flags, trips, 1, 1, 2)
    assert flags[1] == twin.NONE
    twin.arrive(flags, trips, 1, 0, 2)
    assert flags[1] == twin.BOTTOM and trips[1] == 0
    twin.arrive(flags, trips, 1, 1, 2)
    twin.arrive(flags, trips, 1, 0, 2)
    assert trips[1] == 1


def test_swap_uniforms_are_dense_uniform():
    for seed, t, rep in ((0, 0, 0), (12345, 7, 1), (2 ** 40 + 3, 99, 2)):
        i = np.arange(9)
        want = np.array([ora.dense_uniform(k, t, seed, rep) for k in i])
        assert np.array_equal(twin.uniform53(i, t, twin.TAG_DENSE | (rep << 8), seed), want)
        u = twin.swap_uniforms(10, t, seed, rep & 1)
        assert np.array_equal(u, twin.uniform53(i, t, twin.TAG_PT_SWAP | ((rep & 1) << 8), seed))
        assert ((u >= 0) & (u < 1)).all() and not np.array_equal(u, want)
    src = open(os.path.join(ROOT, "tsu-emulator_amd", "csrc", "tsu_common.h")).read()
    assert re.search(r"TSU_TAG_PT_SWAP\s*=\s*8\b", src)


# ---------------------------------------------------------------- validation before the device is touched
@pytest.fixture
def no_device(monkeypatch):
    from tsu import _hip

    def boom(*a, **k):
        raise AssertionError("the device was touched before validation")
    monkeypatch.setattr(_hip, "TemperingLattice", boom)
    monkeypatch.setattr(_hip, "Lattice", boom)
    return _hip


def _open(rows, cols, periodic=True):
    jr, jd, _ = twin.disorder_twin.uniform_disorder(rows, cols, periodic, 1.0)
    return jr, jd


@pytest.mark.parametrize("kw", [
    dict(temperatures=[1.0]),
    dict(temperatures=np.linspace(0.5, 2.0, 257)),
    dict(temperatures=[1.0, 0.0]),
    dict(temperatures=[1.0, np.nan]),
    dict(temperatures=[1.0, np.inf]),
    dict(ladders=3),
    dict(initial="sideways"),
    dict(couplings=_open(8, 8), coupling=2.0),
    dict(field=np.zeros((8, 8)), external_field=0.5),
    dict(couplings=_open(8, 6)),
    dict(field=np.full((8, 8), np.nan)),
    dict(couplings=(np.ones((8, 8)), np.ones((8, 8))), periodic=False),
])
def test_tempering_validation_precedes_device(no_device, kw):
    from tsu.models.ising import LatticeTempering
    args = dict(temperatures=[0.5, 1.0, 2.0], seed=1)
    args.update(kw)
    with pytest.raises(ValueError):
        LatticeTempering(8, args.pop("temperatures"), **args)


def test_tempering_scan_validation_precedes_device(no_device):
    from tsu.models.ising import tempering_scan
    jr, jd = _open(8, 8)
    with pytest.raises(ValueError):
        tempering_scan(8, [1.0, 2.0], couplings=(jr, jd), replicas=3)
    with pytest.raises(ValueError, match="multiple of measure_every"):
        tempering_scan(8, [1.0, 2.0], couplings=(jr, jd), n_equilibrate=15, measure_every=10)
    with pytest.raises(ValueError):
        tempering_scan(8, [1.0, 2.0], couplings=(jr, jd), bias_mode="compat")
    with pytest.raises(ValueError):
        tempering_scan(8, [1.0, 2.0], field=np.zeros((4, 8)))
    with pytest.raises(ValueError):
        tempering_scan(8, [1.0, 2.0], couplings=(jr, jd), coupling=2.0)


def test_symbols_in_header_and_library():
    from tsu import _hip
    header = open(os.path.join(ROOT, "include", "tsu_hip.h")).read()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for n in PT_SYMBOLS:
        assert re.search(rf"\b{n}\s*\(", header), n
        assert hasattr(lib, n), n
        assert n in _hip.SIGNATURES, n
    from tsu.models import LatticeTempering, tempering_scan  # noqa: F401

"""Population annealing without a GPU: the twin's integer resampler (tests/helpers/population_twin.py), its batched restatement of the
lattice twins' sweeps, the estimators of tsu.models.ising on synthetic records, the C ABI's header / ctypes agreement, and argument
validation before any device call."""
import ctypes
import importlib.util
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_spec = importlib.util.spec_from_file_location("population_twin", os.path.join(HERE, "helpers", "population_twin.py"))
twin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(twin)

NEW_SYMBOLS = [pre + name for pre in ("tsu_pa2d_", "tsu_pa3d_")
               for name in ("create", "destroy", "set_disorder", "set_schedule", "init", "run", "history", "energies", "get_spins",
                            "set_spins", "launch_count")]


def _weights(R, db, seed):
    E = np.random.default_rng(seed).normal(size=R) * 4.0
    return twin.weights(E, db)[0]


@pytest.mark.parametrize("R", [2, 3, 64, 65, 257, 1025])
@pytest.mark.parametrize("db", [1e-9, 0.3, 5.0])
def test_resampler_counts_and_placement(R, db):
    W = _weights(R, db, R)
    S = sum(W)
    assert max(W) == twin.ONE
    for k_abs in (0, 1, 7):
        r = twin.resample(W, k_abs, seed=99)
        n, parent = r["n"], r["parent"]
        assert 0 <= r["U"] < S
        assert sum(n) == R
        for i, (x, w) in enumerate(zip(n, W)):
            q = Fraction(R * w, S)
            assert x in (math.floor(q), math.ceil(q)), (i, x, q)
        _, dead, extra = twin.placement(n)
        assert dead == sorted(dead) and extra == sorted(extra)
        assert all(n[d] == 0 for d in dead) and all(n[g] >= 2 for g in extra)
        for i in range(R):  # survivors are fixed points, the dead take the extras in order
            assert parent[i] == (i if n[i] >= 1 else extra[dead.index(i)])
        assert np.array_equal(np.bincount(parent, minlength=R), n)
    if db == 1e-9:
        assert parent == list(range(R))


def test_resampler_by_hand():
    """R = 4, W = (4, 0, 1, 3), S = 8: R C = (16, 16, 20, 32).  U = 3: (19, 19, 23, 35) // 8 = (2, 2, 2, 4), n = (2, 0, 0, 2): the
    dead 1, 2 take the extras 0, 3.  U = 7: (23, 23, 27, 39) // 8 = (2, 2, 3, 4), n = (2, 0, 1, 1): walker 1 takes a copy of 0."""
    W = [4, 0, 1, 3]
    assert twin.counts(W, 3) == [2, 0, 0, 2]
    assert twin.placement([2, 0, 0, 2]) == ([0, 0, 3, 3], [1, 2], [0, 3])
    assert twin.counts(W, 7) == [2, 0, 1, 1]
    assert twin.placement([2, 0, 1, 1])[0] == [0, 0, 2, 3]
    assert twin.counts(W, 0) == [2, 0, 0, 2]


def test_equal_weights_give_the_identity():
    for R in (2, 5, 64, 1000):
        W = [twin.ONE] * R
        for U in (0, 1, R * twin.ONE - 1):
            assert twin.counts(W, U) == [1] * R
        assert twin.resample(W, 3, 5)["parent"] == list(range(R))
    assert twin.weights(np.full(7, -3.25), 0.7) == ([twin.ONE] * 7, -3.25)


def test_offset_is_mulhi_of_the_philox_words():
    cl = twin._load("cluster_twin")
    for seed, k in ((0, 0), (12345678901234, 5), ((1 << 63) + 17, 3)):
        w = cl.philox4x32_10(0, 0, k, twin.TAG_POP_RESAMPLE, seed & 0xFFFFFFFF, seed >> 32)
        x64 = (int(w[1]) << 32) | int(w[0])
        for S in (twin.ONE, 3 * twin.ONE + 12345, (1 << 46) - 1):
            assert twin.offset(S, k, seed) == (x64 * S) >> 64 < S


@pytest.mark.parametrize("shape,periodic", [((12, 20), False), ((16, 16), True), ((5, 37), False)])
def test_batched_sweeps_are_disorder_twins(shape, periodic):
    rng = np.random.default_rng(shape[1])
    jr, jd, h = (rng.normal(size=shape).astype(np.float32) for _ in range(3))
    if not periodic:
        jr[:, -1] = 0
        jd[-1, :] = 0
    seed, B = (1 << 33) + 5, 4
    s0 = twin.initial_spins(shape, seed, B)
    got = twin.sweep_batch(s0, periodic, (jr, jd, h), 1.3, 2, [seed + i for i in range(B)], 3)
    for i in range(B):
        want = twin.disorder_twin.sweep(s0[i], periodic, jr, jd, h, 1.3, 2, seed + i, 3, 0)
        assert (got[i] == want).all(), i


@pytest.mark.parametrize("shape,periodic", [((3, 4, 6), (False, True, True)), ((3, 5, 18), False), ((4, 2, 2), (True, False, False))])
def test_batched_sweeps_are_lattice3d_twins(shape, periodic):
    rng = np.random.default_rng(shape[2])
    dis = [rng.normal(size=shape).astype(np.float32) for _ in range(4)]
    for a, ax, p in zip(dis[:3], (2, 1, 0), twin.lattice3d_twin.axes(periodic)[::-1]):
        if not p:
            np.moveaxis(a, ax, 0)[-1] = 0
    seed, B = 77, 3
    s0 = twin.initial_spins(shape, seed, B)
    got = twin.sweep_batch(s0, periodic, tuple(dis), 0.8, 2, [seed + i for i in range(B)], 1)
    for i in range(B):
        want = twin.lattice3d_twin.sweep(s0[i], periodic, *dis, 0.8, 2, seed + i, 1, 0)
        assert (got[i] == want).all(), i


def test_free_energy_on_a_synthetic_record():
    """Two-level system of N = 3 spins, degenerate: every walker has E = 0 at every step.  Then W = 2^30, S = R 2^30, ln Q = 0 and
    ln Z stays N ln 2, F = -N ln 2 / beta, entropy = N ln 2.  With E_min = -2 throughout and S = R 2^30 / 2 at a step of db = 0.5:
    ln Q = 1 - ln 2."""
    from tsu.models import ising
    betas = np.array([0.0, 0.5, 1.0])
    R = 8
    out = ising.population_free_energy(betas, [R * twin.ONE] * 2, [0.0, 0.0], [0.0] * 3, R, 3)
    np.testing.assert_allclose(out["ln_Z"], 3 * np.log(2.0), rtol=1e-15)
    assert np.isnan(out["F"][0])
    np.testing.assert_allclose(out["F"][1:], -3 * np.log(2.0) / betas[1:], rtol=1e-15)
    np.testing.assert_allclose(out["entropy"], 3 * np.log(2.0), rtol=1e-15)
    out = ising.population_free_energy(betas, [R * twin.ONE // 2] * 2, [-2.0, -2.0], [-1.0, -1.5, -1.75], R, 3)
    np.testing.assert_allclose(out["ln_Q"], 1.0 - np.log(2.0), rtol=1e-15)
    np.testing.assert_allclose(out["ln_Z"], 3 * np.log(2.0) + np.arange(3) * (1.0 - np.log(2.0)), rtol=1e-15)
    np.testing.assert_allclose(out["entropy"], betas * np.array([-1.0, -1.5, -1.75]) + out["ln_Z"], rtol=1e-15)
    # beta[0] > 0: differences only
    out = ising.population_free_energy(betas + 0.25, [R * twin.ONE // 2] * 2, [-2.0, -2.0], [-1.0, -1.5, -1.75], R, 3)
    np.testing.assert_allclose(out["ln_Z"], np.arange(3) * (1.0 - np.log(2.0)), rtol=1e-15)
    assert np.all(np.isnan(out["F"])) and np.all(np.isnan(out["entropy"]))


def test_family_stats_on_a_synthetic_record():
    from tsu.models import ising
    parent = np.array([[0, 0, 2, 3], [0, 1, 2, 2], [0, 1, 2, 3]])
    out = ising.population_family_stats(parent)
    # families by walker: (0, 1, 2, 3) -> (0, 0, 2, 3) -> (0, 0, 2, 2) -> the same
    np.testing.assert_array_equal(out["families"], [4, 3, 2, 2])
    np.testing.assert_allclose(out["rho_t"], [1.0, 4 * (0.25 + 2 / 16), 2.0, 2.0], rtol=1e-15)
    np.testing.assert_allclose(out["rho_s"], [4.0, np.exp(-(0.5 * np.log(0.5) + 0.5 * np.log(0.25))), 2.0, 2.0], rtol=1e-15)


def test_header_and_ctypes_prototypes_agree():
    """The entry points are declared in include/tsu_hip_population.h, which tsu_hip.h includes, exported by the library, and
    prototyped one to one in _hip.POPULATION_SIGNATURES (which load_library declares); the new Philox tag is 11."""
    from tsu import _hip
    with open(os.path.join(ROOT, "include", "tsu_hip.h")) as f:
        assert re.search(r'^#include "tsu_hip_population.h"', f.read(), flags=re.M)
    with open(os.path.join(ROOT, "include", "tsu_hip_population.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tsu_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_hip.POPULATION_SIGNATURES)
    lib = _hip.load_library()
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW_SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_hip.POPULATION_SIGNATURES[name][1]), name
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == _hip.POPULATION_SIGNATURES[name][1]
    with open(os.path.join(ROOT, "tsu-emulator_amd", "csrc", "tsu_common.h")) as f:
        assert re.search(r"TSU_TAG_POP_RESAMPLE\s*=\s*11\b", f.read()) and twin.TAG_POP_RESAMPLE == 11
    build = open(os.path.join(ROOT, "tsu-emulator_amd", "csrc", "build.sh")).read()
    for header_name in ("pop_dev.h", "pop_host.h", "tsu_hip_population.h"):
        assert header_name in build, header_name
    assert _hip.POPULATION_MAX == 65535


def test_python_surface():
    import tsu
    from tsu import models
    from tsu.models import ising
    for name in ("PopulationAnnealing", "PopulationAnnealing3D", "population_annealing_scan", "population_annealing_scan_3d"):
        assert name in models.__all__ and hasattr(models, name)
    assert tsu.PopulationAnnealing is ising.PopulationAnnealing and tsu.PopulationAnnealing3D is ising.PopulationAnnealing3D
    for cls in (ising.PopulationAnnealing, ising.PopulationAnnealing3D):
        for m in ("run", "history", "free_energy", "observables", "family_stats", "spins", "energies"):
            assert callable(getattr(cls, m)), m
        assert isinstance(cls.sweep_count, property)
    import inspect
    for fn in (ising.population_annealing_scan, ising.population_annealing_scan_3d):
        assert inspect.signature(fn).parameters["external_field"].default == 0.0


def test_arguments_are_refused_before_any_device_call(monkeypatch):
    from tsu import _hip
    from tsu.models import ising

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_hip, "load_library", no_device)
    monkeypatch.setattr(_hip.Context, "default", classmethod(no_device))
    ok = dict(betas=[0.0, 0.5, 1.0])
    for make, size, size_bad_j in ((ising.PopulationAnnealing, 8, (np.ones((8, 8)),)),
                                   (ising.PopulationAnnealing3D, (4, 4, 4), (np.ones((4, 4, 4)),))):
        for pop in (1, 65536, 0, -5, 2.5, True):
            with pytest.raises(ValueError, match="population"):
                make(size, pop, **ok)
        for betas in ([0.0, 0.5, 0.5], [0.0, 1.0, 0.5], [-0.1, 0.5], [0.0, np.inf], [0.0, np.nan], [0.5]):
            with pytest.raises(ValueError, match="betas|at least two"):
                make(size, 16, betas=betas)
        for temps in ([1.0, 2.0], [np.inf, np.inf, 1.0], [2.0, 0.0], [2.0, -1.0]):
            with pytest.raises(ValueError, match="decrease|positive|betas"):
                make(size, 16, temperatures=temps)
        with pytest.raises(ValueError, match="exactly one"):
            make(size, 16)
        with pytest.raises(ValueError, match="exactly one"):
            make(size, 16, betas=[0.0, 1.0], temperatures=[np.inf, 1.0])
        with pytest.raises(ValueError, match="sweeps"):
            make(size, 16, sweeps_per_step=-1, **ok)
        with pytest.raises(ValueError):  # the ladders' disorder validation
            make(size, 16, couplings=size_bad_j, **ok)
    with pytest.raises(_hip.UnsupportedError, match="periodic axis"):
        ising.PopulationAnnealing3D((4, 3, 4), 16, **ok)
    np.testing.assert_array_equal(ising._population_schedule(None, [np.inf, 2.0, 0.5]), [0.0, 0.5, 2.0])


def test_n_steps_past_the_schedule_is_refused_on_the_host():
    from tsu.models import ising

    class Handle:  # stands in for the device handle: any call fails the test
        step_count = 1

        def __getattr__(self, name):
            raise AssertionError("a device call was made: " + name)
    pa = ising.PopulationAnnealing.__new__(ising.PopulationAnnealing)
    pa.betas, pa.sweeps_per_step, pa._pa = np.array([0.0, 0.5, 1.0]), 2, Handle()
    for n in (2, 3, -1):
        with pytest.raises(ValueError, match="past the schedule"):
            pa.run(n)

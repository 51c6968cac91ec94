"""Tempering ensembles without a GPU: the disorder-sample generator, the disorder averages of ensemble_summary against direct NumPy
(the jackknife error of the Binder ratio for five samples worked out by hand), the seed rule, the argument validation that happens
before a handle is made, and the C ABI's header / ctypes agreement."""
import ctypes
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

NEW_SYMBOLS = [pre + name for pre in ("tsu_pte2d_", "tsu_pte3d_") for name in (
    "create", "destroy", "set_disorder", "set_temperatures", "init", "run", "history", "stats", "energies", "get_spins", "set_spins",
    "launch_count", "set_correlation", "history_modes", "set_link_overlap", "history_link", "profiles")]


# ---------------------------------------------------------------- edwards_anderson_samples
@pytest.mark.parametrize("size,dims,shape", [(4, 3, (4, 4, 4)), ((3, 5, 7), 3, (3, 5, 7)), (6, 2, (6, 6)), ((5, 9), 2, (5, 9))])
@pytest.mark.parametrize("kind", ["bimodal", "gaussian"])
def test_samples_shape_dtype_and_values(size, dims, shape, kind):
    from tsu.models import edwards_anderson_samples
    js = edwards_anderson_samples(size, 5, kind=kind, seed=3, dims=dims)
    assert isinstance(js, tuple) and len(js) == dims
    for a in js:
        assert a.shape == (5,) + shape and a.dtype == np.float32 and np.isfinite(a).all()
        if kind == "bimodal":
            assert set(np.unique(a)) == {-1.0, 1.0}
        else:
            assert len(np.unique(a)) > a.size // 2 and abs(float(a.mean())) < 0.2
    assert not np.array_equal(js[0][0], js[0][1]) and not np.array_equal(js[0][0], js[1][0])


def test_samples_are_reproducible_and_independent_of_their_number():
    from tsu.models import edwards_anderson_samples
    a = edwards_anderson_samples((3, 4, 6), 6, kind="gaussian", seed=9)
    b = edwards_anderson_samples((3, 4, 6), 6, kind="gaussian", seed=9)
    few = edwards_anderson_samples((3, 4, 6), 2, kind="gaussian", seed=9)
    other = edwards_anderson_samples((3, 4, 6), 2, kind="gaussian", seed=10)
    for x, y, f, o in zip(a, b, few, other):
        assert np.array_equal(x, y) and np.array_equal(x[:2], f) and not np.array_equal(f, o)
    # the documented draw: sample s from default_rng([seed, s]) in the order J_right, J_down, J_layer
    rng = np.random.default_rng([9, 4])
    for x in a:
        assert np.array_equal(x[4], rng.standard_normal((3, 4, 6)).astype(np.float32))
    rng = np.random.default_rng([0, 1])
    bim = edwards_anderson_samples((4, 6), 2, dims=2)
    for x in bim:
        assert np.array_equal(x[1], (2.0 * rng.integers(0, 2, size=(4, 6)) - 1.0).astype(np.float32))


def test_samples_open_boundary_bonds_are_zero_and_the_rest_unchanged():
    from tsu.models import edwards_anderson_samples
    full = edwards_anderson_samples((3, 4, 6), 2, seed=1)
    jr, jd, jl = edwards_anderson_samples((3, 4, 6), 2, seed=1, periodic=(False, True, False))
    assert not jr[..., -1].any() and not jl[:, -1].any() and jd[:, :, -1].all()
    assert np.array_equal(jr[..., :-1], full[0][..., :-1]) and np.array_equal(jl[:, :-1], full[2][:, :-1]) and np.array_equal(jd, full[1])
    j2 = edwards_anderson_samples((4, 6), 2, dims=2, periodic=False)
    assert not j2[0][..., -1].any() and not j2[1][:, -1].any()
    for bad in (dict(dims=4), dict(kind="uniform"), dict(n_samples=0), dict(periodic=(True, False))):
        kw = dict(size=4, n_samples=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            edwards_anderson_samples(**kw)


# ---------------------------------------------------------------- ensemble_summary
def test_summary_against_direct_numpy():
    from tsu.models.ising import correlation_length, ensemble_summary
    rng = np.random.default_rng(0)
    S, R = 7, 4
    smp = {"energy": rng.normal(size=(S, R)), "overlap": rng.random((S, R)), "overlap_sq": rng.random((S, R)) + 0.5,
           "overlap_4": rng.random((S, R)) + 1.0, "link_overlap": rng.random((S, R)), "f2": 4096.0 * (rng.random((S, R)) + 2.0),
           "F2": np.concatenate([np.full((S, R, 1), np.nan), 512.0 * (rng.random((S, R, 2)) + 1.0)], axis=2)}
    N, L, per = 64, (4, 4, 4), (False, True, True)
    out = ensemble_summary(smp, N, L, per)
    for k in ("energy", "overlap", "overlap_sq", "link_overlap"):
        assert np.allclose(out[k], smp[k].mean(axis=0), rtol=1e-14)
        assert np.allclose(out[k + "_err"], smp[k].std(axis=0, ddof=1) / np.sqrt(S), rtol=1e-13)
    q4, q2 = smp["overlap_4"].mean(axis=0), smp["overlap_sq"].mean(axis=0)
    assert np.allclose(out["binder"], 0.5 * (3 - q4 / q2 ** 2), rtol=1e-14)  # averaged first, divided afterwards
    assert not np.allclose(out["binder"], (0.5 * (3 - smp["overlap_4"] / smp["overlap_sq"] ** 2)).mean(axis=0), rtol=1e-6)
    F2, f2 = smp["F2"].mean(axis=0), smp["f2"].mean(axis=0)
    assert np.allclose(out["chi_k"], F2 / N, rtol=1e-14, equal_nan=True) and np.isnan(out["chi_k"][:, 0]).all()
    xi = correlation_length(f2, F2, L)
    assert np.allclose(out["xi"], xi, rtol=1e-14, equal_nan=True)
    assert np.allclose(out["xi_over_L"], (xi[:, 1:] / 4.0).mean(axis=1), rtol=1e-14)
    # the jackknife of xi / L, restated: delete one sample, average, take the ratio
    th = np.stack([(correlation_length(np.delete(smp["f2"], i, 0).mean(axis=0), np.delete(smp["F2"], i, 0).mean(axis=0), L)[:, 1:] / 4.0
                    ).mean(axis=1) for i in range(S)])
    assert np.allclose(out["xi_over_L_err"], np.sqrt((S - 1) / S * ((th - th.mean(axis=0)) ** 2).sum(axis=0)), rtol=1e-12)
    one = ensemble_summary({k: v[:1] for k, v in smp.items()}, N, L, per)
    assert np.isnan(one["energy_err"]).all() and np.isnan(one["binder_err"]).all() and np.allclose(one["energy"], smp["energy"][0])
    with pytest.raises(ValueError):
        ensemble_summary(smp)
    assert set(ensemble_summary({"energy": smp["energy"]})) == {"energy", "energy_err"}


def test_binder_jackknife_by_hand():
    """S = 5, one temperature: <q^2> = 1 for every sample and <q^4> = 1, 2, 3, 4, 5.  [q^4] = 3, so binder = (3 - 3) / 2 = 0.
    Deleting sample i leaves [q^4]_(i) = (15 - q4_i) / 4 = 3.5, 3.25, 3, 2.75, 2.5, so theta_i = (3 - [q^4]_(i)) / 2 =
    -0.25, -0.125, 0, 0.125, 0.25 with mean 0; sum of squares = 2 (1/16 + 1/64) = 5/32; error = sqrt(4/5 * 5/32) = sqrt(1/8)."""
    from tsu.models.ising import ensemble_summary
    out = ensemble_summary({"overlap_sq": np.ones((5, 1)), "overlap_4": np.arange(1.0, 6.0).reshape(5, 1)})
    assert out["binder"][0] == 0.0
    assert abs(out["binder_err"][0] - np.sqrt(1.0 / 8.0)) < 1e-15
    assert out["overlap_sq"][0] == 1.0 and out["overlap_sq_err"][0] == 0.0


# ---------------------------------------------------------------- seeds and validation before any handle
def test_seed_rule():
    from tsu.models.ising import ensemble_seeds
    assert ensemble_seeds(100, 4, 2, 5) == [100, 110, 120, 130]
    assert ensemble_seeds(2 ** 40, 3, 1, 256) == [2 ** 40, 2 ** 40 + 256, 2 ** 40 + 512]
    keys = [s + i for s in ensemble_seeds(7, 6, 2, 3) for i in range(6)]  # walker (s, k, w): seeds[s] + k R + w
    assert len(set(keys)) == len(keys) == 36


@pytest.fixture
def no_handles(monkeypatch):
    """Any attempt to make a device handle fails the test: the validation under test must come first."""
    from tsu import _hip

    def refuse(*a, **k):
        raise AssertionError("a device handle was requested before the arguments were validated")
    for name in ("TemperingEnsemble", "TemperingEnsemble3D", "TemperingLattice", "TemperingLattice3D"):
        monkeypatch.setattr(_hip, name, refuse)
    monkeypatch.setattr(_hip.Context, "default", classmethod(refuse))


def test_validation_before_a_handle(no_handles):
    from tsu import _hip
    from tsu.models.ising import (LatticeTemperingEnsemble, LatticeTemperingEnsemble3D, edwards_anderson_samples,
                                  tempering_ensemble_scan, tempering_ensemble_scan_3d)
    shape, Ts = (4, 4, 6), [0.5, 1.0, 2.0]
    js = edwards_anderson_samples(shape, 3, seed=1)
    h = np.zeros((3,) + shape)
    E3 = LatticeTemperingEnsemble3D
    cases = [
        (dict(couplings=js[:2]), "couplings"),                                     # a pair where a triple is due
        (dict(couplings=tuple(a[0] for a in js)), "shape"),                        # no sample axis
        (dict(couplings=(js[0], js[1], js[2][:2])), "samples"),                    # leading axes differ
        (dict(couplings=js, field=h[:1]), "samples"),
        (dict(couplings=js, field=h[:, :2]), "shape"),
        (dict(couplings=tuple(a[:0] for a in js)), "at least one"),                # S = 0
        (dict(couplings=js, seeds=[1, 2]), "seed"),
        (dict(couplings=js, seeds=[1, 2, 3], seed=4), "seeds"),
        (dict(couplings=js, seeds=[1, 2, -3]), "64-bit"),
        (dict(couplings=js, ladders=3), "ladders"),
        (dict(couplings=js, link_overlap=True), "ladders=2"),
        (dict(couplings=js, initial="hot"), "initial"),
        (dict(couplings=(js[0], js[1], np.where(np.arange(3)[:, None, None, None] == 1, np.inf, js[2]))), "finite"),
        (dict(couplings=js, periodic=False), "open"),                              # non-zero bonds across an open boundary
        (dict(couplings=js, periodic=False, correlation=True), "periodic axis"),
    ]
    for kw, match in cases:
        with pytest.raises(ValueError, match=match):
            E3(shape, Ts, **kw)
    with pytest.raises(_hip.UnsupportedError, match="even length"):
        E3((5, 4, 6), Ts, couplings=edwards_anderson_samples((5, 4, 6), 2))
    with pytest.raises(ValueError, match="temperatures"):
        E3(shape, [1.0], couplings=js)
    # 128 samples x 2 ladders x 256 temperatures = 65536 walkers
    big = edwards_anderson_samples((2, 2, 2), 128, periodic=False)
    with pytest.raises(ValueError, match="65536 walkers"):
        E3((2, 2, 2), np.linspace(0.5, 3.0, 256), couplings=big, periodic=False, ladders=2)
    j2 = edwards_anderson_samples((4, 6), 3, dims=2)
    with pytest.raises(ValueError, match="couplings"):
        LatticeTemperingEnsemble((4, 6), Ts, couplings=js)
    with pytest.raises(ValueError, match="samples"):
        LatticeTemperingEnsemble((4, 6), Ts, couplings=j2, field=np.zeros((2, 4, 6)))
    with pytest.raises(ValueError, match="open"):
        LatticeTemperingEnsemble((4, 6), Ts, couplings=j2, periodic=False)
    for scan, sz, jj in ((tempering_ensemble_scan, (4, 6), j2), (tempering_ensemble_scan_3d, shape, js)):
        with pytest.raises(ValueError, match="replicas"):
            scan(sz, Ts, couplings=jj, replicas=3)
        with pytest.raises(ValueError, match="replicas=2"):
            scan(sz, Ts, couplings=jj, link_overlap=True)
        with pytest.raises(ValueError, match="multiple"):
            scan(sz, Ts, couplings=jj, n_equilibrate=15, measure_every=10)
        with pytest.raises(ValueError, match="periodic axis"):
            scan(sz, Ts, couplings=jj, periodic=False, correlation=True)


def test_python_surface():
    import inspect
    import tsu
    from tsu import models
    from tsu.models import ising
    names = ("LatticeTemperingEnsemble", "LatticeTemperingEnsemble3D", "edwards_anderson_samples", "ensemble_summary",
             "tempering_ensemble_scan", "tempering_ensemble_scan_3d")
    for n in names:
        assert getattr(tsu, n) is getattr(models, n) is getattr(ising, n) and n in tsu.__all__ and n in models.__all__
    want = ["size", "temperatures", "couplings", "field", "periodic", "seeds", "seed", "initial", "ladders", "correlation", "link_overlap"]
    for cls in (ising.LatticeTemperingEnsemble, ising.LatticeTemperingEnsemble3D):
        sig = inspect.signature(cls)
        assert list(sig.parameters) == want
        assert all(p.kind is p.KEYWORD_ONLY for n, p in sig.parameters.items() if n not in ("size", "temperatures"))
        for attr in ("run", "history", "spins", "energy", "acceptance", "acceptance_pooled", "round_trips", "walker_at_slot",
                     "sweep_count", "close"):
            assert hasattr(cls, attr), attr
    assert list(inspect.signature(ising.edwards_anderson_samples).parameters)[:5] == ["size", "n_samples", "kind", "seed", "dims"]


# ---------------------------------------------------------------- header and bindings
def test_header_and_ctypes_prototypes_agree():
    """The entry points are declared in include/tsu_hip_ensemble.h, which tsu_hip.h includes after tsu_hip_overlap.h, exported by the
    library, and prototyped one to one in _hip.ENSEMBLE_SIGNATURES (which load_library declares)."""
    from tsu import _hip
    with open(os.path.join(ROOT, "include", "tsu_hip.h")) as f:
        top = f.read()
    assert re.search(r'^#include "tsu_hip_ensemble.h"', top, flags=re.M)
    assert top.index('#include "tsu_hip_overlap.h"') < top.index('#include "tsu_hip_ensemble.h"')
    with open(os.path.join(ROOT, "include", "tsu_hip_ensemble.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tsu_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_hip.ENSEMBLE_SIGNATURES)
    lib = _hip.load_library()
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW_SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_hip.ENSEMBLE_SIGNATURES[name][1]), name
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == _hip.ENSEMBLE_SIGNATURES[name][1]
    # an ensemble's entry point takes its ladder's arguments plus the sample: one more int in create, get_spins, set_spins, profiles
    for name in NEW_SYMBOLS:
        ladder = name.replace("pte", "pt")
        sigs = {**_hip.SIGNATURES, **_hip.CORRELATION_SIGNATURES, **_hip.OVERLAP_SIGNATURES}
        extra = 1 if name.split("_", 2)[2] in ("create", "get_spins", "set_spins", "profiles") else 0
        assert len(_hip.ENSEMBLE_SIGNATURES[name][1]) == len(sigs[ladder][1]) + extra, name
    older = (set(_hip.SIGNATURES) | set(_hip.CLUSTER3D_SIGNATURES) | set(_hip.CORRELATION_SIGNATURES) | set(_hip.POPULATION_SIGNATURES)
             | set(_hip.OVERLAP_SIGNATURES))
    assert not older & set(NEW_SYMBOLS)
    build = open(os.path.join(ROOT, "tsu-emulator_amd", "csrc", "build.sh")).read()
    for header_name in ("pte_host.h", "tsu_hip_ensemble.h"):
        assert header_name in build, header_name

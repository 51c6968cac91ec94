"""Gaussian-mixture energies on the host: tsu.core.MixtureEnergy against the reference's own values (tests/golden/g13_mixture.npz,
written by tests/golden/make_golden_mixture.py), recognition of the reference's mixture callers, and the CPU twin of the device
kernels (tests/helpers/mixture_twin.py) against the oracle's reference step."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import oracle as ora

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("mixture_twin", os.path.join(HERE, "helpers", "mixture_twin.py"))
twin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(twin)


def _mixture_fn(centers, weights, power=2):
    """E(x) = -log(sum_i w_i exp(-sum_j |x_j - mu_ij|^power / 2) + 1e-10): the stated formula (power 2), vectorised."""
    C = np.asarray(centers, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)

    def energy(x):
        e = np.sum(np.abs(np.atleast_1d(x)[None, :] - C) ** power, axis=1)
        return float(-np.log(np.exp(-0.5 * e) @ w + 1e-10))
    return energy


class _ModeHolder:
    """Recognition's view of the demo distribution: ``mode_centers`` / ``mode_weights`` and a bound ``energy``."""

    def __init__(self, centers, weights, power=2):
        self.mode_centers = np.asarray(centers, dtype=np.float64)
        self.mode_weights = np.asarray(weights, dtype=np.float64)
        self._e = _mixture_fn(self.mode_centers, self.mode_weights, power)
        self.calls = 0

    def energy(self, x):
        self.calls += 1
        return self._e(x)


class _CenterHolder:
    """Recognition's view of the api sampler: ``centers`` (a list of per-component vectors), ``weights`` scaled to sum 1, and a
    bound ``energy_function``."""

    def __init__(self, centers, weights):
        raw = np.asarray(weights, dtype=np.float64)
        self.weights = raw * (1.0 / raw.sum())
        self.centers = list(np.asarray(centers, dtype=np.float64))
        self._e = _mixture_fn(np.stack(self.centers), self.weights)

    def energy_function(self, x):
        return self._e(x)


@pytest.mark.parametrize("which", ["demo", "api"])
def test_mixture_energy_reproduces_the_reference(golden, which):
    from tsu.core import MixtureEnergy
    g = golden("g13_mixture")
    e = MixtureEnergy(g[which + "_centers"], g[which + "_weights"])
    X, E, G = g[which + "_x"], g[which + "_energy"], g[which + "_grad"]
    got = np.array([e(x) for x in X])
    np.testing.assert_allclose(got, E, rtol=1e-12, atol=0)
    grad = np.array([e.gradient(x) for x in X])
    np.testing.assert_allclose(grad, G, rtol=0, atol=1e-6)
    # the plateau: at x = 0 the demo's chains start where p(x) is far below eps
    if which == "demo":
        assert abs(e(np.zeros(10)) - float(g["demo_energy_at_zero"])) <= 1e-12 * abs(float(g["demo_energy_at_zero"]))


def test_mixture_energy_log_domain_far_field():
    """eps = 0 far from every centre: the naive sum underflows to log(0); the log domain keeps a finite pull to the nearest centre."""
    from tsu.core import MixtureEnergy
    c = np.array([[0.0, 0.0], [3.0, 0.0]])
    e = MixtureEnergy(c, [1.0, 1.0], eps=0.0)
    x = np.array([-30.0, 0.0])
    assert np.isfinite(e(x)) and abs(e(x) - (0.5 * 900.0 - np.log(1.0 + np.exp(-0.5 * (33.0 ** 2 - 900.0))))) < 1e-9
    g = e.gradient(x)
    np.testing.assert_allclose(g, x - c[0], rtol=1e-12)
    # sigma per component: E = -log(sum w_i exp(-|x - mu_i|^2 / (2 sigma_i^2)) + eps) (f64 formula at a point where it does not underflow)
    e2 = MixtureEnergy(c, [0.3, 2.0], sigma=[0.5, 2.0], eps=1e-6)
    y = np.array([1.0, 0.7])
    want = -np.log(0.3 * np.exp(-np.sum((y - c[0]) ** 2) / 0.5) + 2.0 * np.exp(-np.sum((y - c[1]) ** 2) / 8.0) + 1e-6)
    assert abs(e2(y) - want) <= 1e-13 * abs(want)
    h = 1e-6
    fd = np.array([(e2(y + h * np.eye(2)[i]) - e2(y - h * np.eye(2)[i])) / (2 * h) for i in range(2)])
    np.testing.assert_allclose(e2.gradient(y), fd, atol=1e-7)


def test_mixture_energy_validation():
    from tsu.core import ConfigurationError, MixtureEnergy
    c = np.zeros((2, 3))
    with pytest.raises(ConfigurationError, match="centers of shape"):
        MixtureEnergy(np.zeros(3), [1.0])
    with pytest.raises(ConfigurationError, match="weights of shape"):
        MixtureEnergy(c, [1.0, 1.0, 1.0])
    with pytest.raises(ConfigurationError, match="weights > 0"):
        MixtureEnergy(c, [1.0, 0.0])
    with pytest.raises(ConfigurationError, match="weights > 0"):
        MixtureEnergy(c, [1.0, np.nan])
    with pytest.raises(ConfigurationError, match="sigma > 0"):
        MixtureEnergy(c, [1.0, 1.0], sigma=[1.0, -1.0])
    with pytest.raises(ConfigurationError, match="sigma as a scalar"):
        MixtureEnergy(c, [1.0, 1.0], sigma=[1.0, 1.0, 1.0])
    with pytest.raises(ConfigurationError, match="eps >= 0"):
        MixtureEnergy(c, [1.0, 1.0], eps=-1e-3)
    with pytest.raises(ConfigurationError, match="finite centers"):
        MixtureEnergy(np.array([[0.0, np.inf, 0.0], [0.0, 0.0, 0.0]]), [1.0, 1.0])
    with pytest.raises(ConfigurationError, match="at most 64 components"):
        MixtureEnergy(np.zeros((65, 3)), np.ones(65))


def test_recognition_admits_both_spellings_and_leaves_np_random_alone():
    from tsu.core import MixtureEnergy, _recognise_mixture
    rng = np.random.default_rng(3)
    demo = _ModeHolder(rng.standard_normal((3, 10)) * 3, [0.3, 0.5, 0.2])
    api = _CenterHolder([[0.0, 0.0], [3.0, 3.0], [-2.0, 4.0]], [1.0, 2.0, 3.0])
    np.random.seed(123)
    before = np.random.get_state()
    m = _recognise_mixture(demo.energy, np.random.RandomState(1).randn(10) * 0.5)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert isinstance(m, MixtureEnergy) and m.eps == 1e-10 and np.all(m.sigma == 1.0)
    np.testing.assert_array_equal(m.centers, demo.mode_centers)
    np.testing.assert_array_equal(m.weights, demo.mode_weights)
    a = _recognise_mixture(api.energy_function, np.zeros(2))
    assert isinstance(a, MixtureEnergy)
    np.testing.assert_array_equal(a.weights, api.weights)
    e = MixtureEnergy(np.zeros((1, 4)), [2.0])
    assert _recognise_mixture(e, np.zeros(4)) is e
    # one component: still checked at 8 points or more
    one = _ModeHolder(np.ones((1, 4)), [1.0])
    assert isinstance(_recognise_mixture(one.energy, np.zeros(4)), MixtureEnergy) and one.calls >= 8


def test_recognition_refuses_what_it_does_not_reproduce():
    from tsu.core import _recognise_mixture
    rng = np.random.default_rng(4)
    c = rng.standard_normal((3, 5)) * 2
    assert _recognise_mixture(_ModeHolder(c, [0.3, 0.5, 0.2], power=3).energy, np.zeros(5)) is None  # a different exponent
    assert _recognise_mixture(_ModeHolder(c, [0.3, 0.5]).energy, np.zeros(5)) is None               # weights of another shape
    assert _recognise_mixture(_ModeHolder(c, [0.3, 0.5, 0.2]).energy, np.zeros(4)) is None          # centres of another dimension
    f = _mixture_fn(c, [0.3, 0.5, 0.2])
    assert _recognise_mixture(lambda x: f(x), np.zeros(5)) is None                           # a lambda: no owner to read


def test_unrecognised_large_callable_message_names_both_descriptors():
    from tsu.core import SamplingError, ThermalSamplingUnit, TSUConfig
    t = ThermalSamplingUnit(TSUConfig(n_burnin=1, n_steps=1), seed=1)
    with pytest.raises(SamplingError, match="MixtureEnergy"):
        t.sample_from_energy(lambda x: float(np.sum(np.abs(x))), np.ones(5000))


def test_twin_single_step_is_the_reference_step():
    """One twin step = the reference's Langevin step (core.py:64-80) with the analytic gradient and the same normals, to f32 rounding."""
    from tsu.core import MixtureEnergy
    ora.build()
    rng = np.random.default_rng(5)
    for d, K, eps, sigma in ((10, 3, 1e-10, 1.0), (7, 5, 0.0, np.linspace(0.5, 2.0, 5)), (1, 1, 1e-3, 0.7)):
        c = rng.standard_normal((K, d)) * 2
        w = rng.uniform(0.1, 2.0, K)
        c32, lw, iv, leps = twin.device_params(c, w, sigma, eps)
        # the energy the device holds, in float64
        e = MixtureEnergy(c32.astype(np.float64), np.exp(lw.astype(np.float64)), 1.0 / np.sqrt(iv.astype(np.float64)),
                          float(np.exp(np.float64(leps))))
        x = (rng.standard_normal((4, d)) * 1.5).astype(np.float32)
        T, dt, gamma = 0.8, 0.01, 1.3
        got = twin.mixture_f32(x, c, w, sigma, eps, 1, dt, gamma, T, seed=9, step0=3, chain0=2)
        xi = twin.normals(4, d, 3, 9, chain0=2).astype(np.float64)
        for n in range(4):
            want = ora.ref_langevin_step(x[n].astype(np.float64), e.gradient(x[n].astype(np.float64)), xi[n], T, dt, gamma)
            np.testing.assert_allclose(got[n], want, rtol=2e-6, atol=2e-7)

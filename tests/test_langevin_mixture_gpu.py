"""K3, Gaussian-mixture energies (csrc/langevin.hip k3_mixture_lane for dim <= 64, k3_mixture_wg above) against the CPU twin
(tests/helpers/mixture_twin.py: the oracle's Philox normals, gradient in float64 from the float32 state and parameters, rounded
once).  The device forms the distances, the log-sum-exp and the gradient in float32 in its own order.  Tolerance 2e-4 (1 + |x|)
absolute (the separable kernel's figure) up to dim 64; above, 1e-3 (1 + |x|): a distance there is a float32 sum of thousands of
terms, of size up to ~1e3, so a_i carries an absolute error of ~1e-4 .. 1e-3, which moves c_i (and the step) by that fraction
wherever two components compete."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import oracle as ora

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("mixture_twin", os.path.join(HERE, "helpers", "mixture_twin.py"))
twin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(twin)


def _tol(d):
    return 2e-4 if d <= 64 else 1e-3


def _problem(d, K, chains, seed):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(d)
    c = base[None, :] + (1.5 / np.sqrt(d)) * rng.standard_normal((K, d))  # centres ~2 apart whatever d is
    w = rng.uniform(0.2, 2.0, K)
    x0 = (c[np.arange(chains) % K] + (0.5 / np.sqrt(d)) * rng.standard_normal((chains, d))).astype(np.float32)
    return c, w, x0


CASES = [  # (dim, K, chains, eps, sigma non-uniform)
    (1, 1, 1, 1e-10, False), (1, 3, 300, 0.0, True), (10, 3, 5, 1e-10, False), (10, 16, 300, 0.0, True),
    (64, 16, 5, 1e-10, True), (64, 3, 300, 0.0, False), (64, 1, 1, 0.0, True),
    (65, 3, 5, 0.0, True), (65, 16, 1, 1e-10, False), (1027, 3, 5, 1e-10, True), (1027, 16, 1, 0.0, True),
    (1027, 1, 5, 0.0, False), (4096, 3, 1, 0.0, True), (4096, 16, 5, 1e-10, True),
    (20000, 3, 2, 0.0, True), (40000, 2, 2, 1e-10, False),  # (8 and 16 quads per lane; centres from L2 at 40000)
]


@pytest.mark.parametrize("d,K,chains,eps,nonuni", CASES)
def test_mixture_steps_match_the_twin(d, K, chains, eps, nonuni):
    from tsu import _hip
    c, w, x0 = _problem(d, K, chains, 1000 * d + K)
    sigma = np.linspace(0.7, 1.4, K) if nonuni else 1.0
    lc = _hip.LangevinChains(chains, d)
    lc.set_mixture(c, w, sigma, eps)
    lc.set_state(x0)
    n, T, dt = 16, 0.3, 0.01
    traj = lc.step(n, dt, 1.0, T, 77, step0=4, chain0=2, trajectory=True)
    got = lc.get_state()
    lc.close()
    want, wtraj = twin.mixture_f32(x0, c, w, sigma, eps, n, dt, 1.0, T, 77, step0=4, chain0=2, trajectory=True)
    tol = _tol(d)
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got - want) <= tol * (1.0 + np.abs(want))), float(np.max(np.abs(got - want)))
    assert np.all(np.abs(traj - wtraj) <= tol * (1.0 + np.abs(wtraj)))
    np.testing.assert_array_equal(traj[-1], got)


@pytest.mark.parametrize("d", [10, 64, 65, 1027])
def test_one_unit_component_is_the_separable_kernel_bit_for_bit(d):
    """K = 1, w = 1, sigma = 1, eps = 0: r = 1, Z = 1, c = 1, g = x - mu -- set_energy(1, mu) bit for bit (same noise, same update)."""
    from tsu import _hip
    rng = np.random.default_rng(d)
    mu = rng.standard_normal(d).astype(np.float32)
    x0 = rng.standard_normal((7, d)).astype(np.float32)
    a = _hip.LangevinChains(7, d)
    a.set_energy(np.ones(d, np.float32), mu)
    a.set_state(x0)
    ta = a.step(25, 0.01, 1.0, 0.9, 31, step0=3, chain0=5, trajectory=True)
    m = _hip.LangevinChains(7, d)
    m.set_mixture(mu[None, :], [1.0], 1.0, 0.0)
    m.set_state(x0)
    tm = m.step(25, 0.01, 1.0, 0.9, 31, step0=3, chain0=5, trajectory=True)
    np.testing.assert_array_equal(tm, ta)
    np.testing.assert_array_equal(m.get_state(), a.get_state())
    # a later set_energy switches the handle back to the separable kernel
    m.set_energy(np.full(d, 2.0, np.float32), mu)
    a.set_energy(np.full(d, 2.0, np.float32), mu)
    m.step(5, 0.01, 1.0, 0.9, 31, step0=28, chain0=5)
    a.step(5, 0.01, 1.0, 0.9, 31, step0=28, chain0=5)
    np.testing.assert_array_equal(m.get_state(), a.get_state())
    a.close()
    m.close()


@pytest.mark.parametrize("d,K", [(10, 3), (40, 9), (300, 5)])
def test_split_launches_and_chain_subsets_are_bit_exact(d, K):
    from tsu import _hip
    c, w, x0 = _problem(d, K, 12, d)
    fused = _hip.LangevinChains(12, d)
    fused.set_mixture(c, w, 0.9, 1e-10)
    fused.set_state(x0)
    tf = fused.step(20, 0.01, 1.0, 0.6, 3, step0=1, chain0=0, trajectory=True)
    split = _hip.LangevinChains(12, d)
    split.set_mixture(c, w, 0.9, 1e-10)
    split.set_kernel(1)
    split.set_state(x0)
    ts = split.step(20, 0.01, 1.0, 0.6, 3, step0=1, chain0=0, trajectory=True)
    np.testing.assert_array_equal(ts, tf)
    np.testing.assert_array_equal(split.get_state(), fused.get_state())
    sub = _hip.LangevinChains(4, d)
    sub.set_mixture(c, w, 0.9, 1e-10)
    sub.set_state(x0[5:9])
    tsub = sub.step(20, 0.01, 1.0, 0.6, 3, step0=1, chain0=5, trajectory=True)
    np.testing.assert_array_equal(tsub, tf[:, 5:9])
    np.testing.assert_array_equal(sub.get_state(), fused.get_state()[5:9])
    for h in (fused, split, sub):
        h.close()


def test_a_larger_mixture_replaces_a_smaller_one():
    """set_mixture with more components than the handle's buffers hold (new buffers) = a fresh handle, bit for bit."""
    from tsu import _hip
    c, w, x0 = _problem(12, 20, 6, 12)
    a = _hip.LangevinChains(6, 12)
    a.set_mixture(c[:2], w[:2], 1.0, 1e-10)
    a.step(3, 0.01, 1.0, 1.0, 9)
    a.set_mixture(c, w, 0.8, 0.0)
    a.set_state(x0)
    a.step(10, 0.01, 1.0, 1.0, 9, step0=3)
    b = _hip.LangevinChains(6, 12)
    b.set_mixture(c, w, 0.8, 0.0)
    b.set_state(x0)
    b.step(10, 0.01, 1.0, 1.0, 9, step0=3)
    np.testing.assert_array_equal(a.get_state(), b.get_state())
    a.close()
    b.close()


def test_plateau_start_and_far_field():
    from tsu import _hip
    # the demo: three modes N(0, 9) in 10-D, weights 0.3 / 0.5 / 0.2, chains started at ~0 where p(x) << eps = 1e-10
    rng = np.random.RandomState(13)
    c = rng.randn(3, 10) * 3
    w = np.array([0.3, 0.5, 0.2])
    x0 = (rng.randn(64, 10) * 0.5).astype(np.float32)
    lc = _hip.LangevinChains(64, 10)
    lc.set_mixture(c, w, 1.0, 1e-10)
    lc.set_state(x0)
    traj = lc.step(30, 0.01, 1.0, 0.5, 8, trajectory=True)
    want, wtraj = twin.mixture_f32(x0, c, w, 1.0, 1e-10, 30, 0.01, 1.0, 0.5, 8, trajectory=True)
    np.testing.assert_allclose(lc.get_state(), want, rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(traj, wtraj, rtol=2e-4, atol=2e-4)
    lc.close()
    # eps = 0, ||x - mu||^2 ~ 900 from the nearest centre: a finite pull toward it (the naive sum would be 0 / 0)
    c2 = np.array([[0.0] * 10, [6.0] * 10])
    x1 = np.full((8, 10), -9.5, np.float32)  # |x - c0|^2 = 902.5
    far = _hip.LangevinChains(8, 10)
    far.set_mixture(c2, [1.0, 1.0], 1.0, 0.0)
    far.set_state(x1)
    far.step(10, 0.01, 1.0, 1e-6, 4)
    x = far.get_state().astype(np.float64)
    far.close()
    assert np.all(np.isfinite(x))
    # deterministic part: x_n = -9.5 (1 - dt)^n toward c0
    np.testing.assert_allclose(x, -9.5 * 0.99 ** 10, rtol=1e-3)


def _grid_density(c, w, sigma, T, lim=7.0, n=701):
    g = np.linspace(-lim, lim, n)
    X, Y = np.meshgrid(g, g, indexing="ij")
    P = np.stack([X.ravel(), Y.ravel()], 1)
    a = np.log(w)[None, :] - 0.5 * np.sum((P[:, None, :] - c[None]) ** 2, axis=2) / sigma[None, :] ** 2
    m = a.max(1, keepdims=True)
    E = -(m[:, 0] + np.log(np.exp(a - m).sum(1)))
    p = np.exp(-(E - E.min()) / T)
    return P, p / p.sum(), g[1] - g[0]


@pytest.mark.parametrize("T", [0.5, 1.0])
def test_stationary_distribution_of_a_two_dimensional_mixture(T):
    from tsu import _hip
    c = np.array([[0.0, 0.0], [1.6, 0.6], [-0.6, 1.5]])
    w = np.array([1.0, 0.7, 0.5])
    sigma = np.array([0.8, 1.0, 0.6])
    P, p, h = _grid_density(c, w, sigma, T)
    n = 8192
    rng = np.random.default_rng(int(T * 10))
    start = P[rng.choice(p.size, size=n, p=p)] + rng.uniform(-h / 2, h / 2, size=(n, 2))  # exact draws of exp(-E/T)
    lc = _hip.LangevinChains(n, 2)
    lc.set_mixture(c, w, sigma, 0.0)
    lc.set_state(start.astype(np.float32))
    lc.step(2000, 0.01, 1.0, T, 1234)
    x = lc.get_state().astype(np.float64)
    lc.close()
    mean = p @ P
    cov = (P - mean).T @ ((P - mean) * p[:, None])
    se = np.sqrt(np.diag(cov) / n)
    assert np.all(np.abs(x.mean(0) - mean) <= 4 * se + 0.01), (x.mean(0), mean)
    xc = np.cov(x.T)
    # (Euler's stationary law is the target's up to O(dt): 1 % of the variances beside the sampling error sqrt(2 / n))
    assert np.all(np.abs(xc - cov) <= 4 * np.sqrt(2.0 / n) * np.sqrt(np.outer(np.diag(cov), np.diag(cov))) + 0.01 * np.max(np.diag(cov))), (xc, cov)
    # histogram: four quadrants around each centre's axis and the far band
    edges = [-np.inf, -0.5, 0.5, 1.5, np.inf]
    for ax in (0, 1):
        want = np.array([p[(P[:, ax] > lo) & (P[:, ax] <= hi)].sum() for lo, hi in zip(edges[:-1], edges[1:])])
        got = np.array([np.mean((x[:, ax] > lo) & (x[:, ax] <= hi)) for lo, hi in zip(edges[:-1], edges[1:])])
        assert np.all(np.abs(got - want) <= 4 * np.sqrt(want * (1 - want) / n) + 0.006), (ax, got, want)


class _ModeHolder:
    """Recognition's view of the demo distribution: ``mode_centers`` / ``mode_weights`` and a bound energy written from the formula
    E(x) = -log(sum_i w_i exp(-||x - mu_i||^2 / 2) + 1e-10)."""

    def __init__(self, dim):
        rng = np.random.default_rng(5)
        self.mode_centers = 3.0 * rng.standard_normal((3, dim))
        self.mode_weights = np.array([0.3, 0.5, 0.2])

    def energy(self, x):
        d2 = np.sum((np.atleast_1d(x)[None, :] - self.mode_centers) ** 2, axis=1)
        return float(-np.log(np.exp(-0.5 * d2) @ self.mode_weights + 1e-10))


@pytest.mark.parametrize("which", ["mixture10", "mixture8192", "demo"])
def test_sample_from_energy_runs_mixtures_on_the_device(which, monkeypatch):
    from tsu.core import MixtureEnergy, ThermalSamplingUnit, TSUConfig

    def no_host(*a, **k):
        raise AssertionError("the host finite-difference loop was entered")

    monkeypatch.setattr(ThermalSamplingUnit, "_numerical_gradient", no_host)
    if which == "demo":
        d = 10
        obj = _ModeHolder(d)
        fn = obj.energy
        c, w, sigma, eps = obj.mode_centers, obj.mode_weights, 1.0, 1e-10
    else:
        d = 10 if which == "mixture10" else 8192
        rng = np.random.default_rng(d)
        c = rng.standard_normal((3, d)) * (3.0 / np.sqrt(d) if d > 64 else 1.0)
        w, sigma, eps = np.array([1.0, 2.0, 0.5]), np.array([1.0, 0.8, 1.2]), 1e-10
        fn = MixtureEnergy(c, w, sigma, eps)
    x_init = np.random.default_rng(1).standard_normal(d) * 0.5
    cfg = TSUConfig(temperature=0.5, n_burnin=10, n_steps=15)
    t = ThermalSamplingUnit(cfg, seed=42)
    samples, traj = t.sample_from_energy(fn, x_init, n_samples=6, return_trajectory=True)
    assert samples.shape == (6, d) and samples.dtype == np.float64
    assert t.sample_count == 6 and len(traj) == 6 * 15
    np.testing.assert_array_equal(traj[cfg.n_steps - 1], samples[0])
    # sample 0 starts exactly at x_init: its first state is one twin step from there (chain id 0, step 0, the seed)
    t0 = ThermalSamplingUnit(TSUConfig(temperature=0.5, n_burnin=0, n_steps=1), seed=42)
    s0 = t0.sample_from_energy(fn, x_init, n_samples=3)
    want = twin.mixture_f32(x_init.astype(np.float32)[None], c, w, sigma, eps, 1, 0.01, 1.0, 0.5, 42, step0=0, chain0=0)
    np.testing.assert_allclose(s0[0], want[0], rtol=0, atol=_tol(d) * (1 + np.max(np.abs(want))))
    assert np.max(np.abs(s0[1] - x_init)) > 1e-3  # the others restart at x_init + 0.1 N(0, 1)
    # seeded reproducibility (and fresh chain ids on a second call)
    again = ThermalSamplingUnit(cfg, seed=42).sample_from_energy(fn, x_init, n_samples=6)
    np.testing.assert_array_equal(again, samples)
    second = t.sample_from_energy(fn, x_init, n_samples=6)
    assert not np.array_equal(second, samples)


def test_set_mixture_refusals():
    from tsu import _hip
    lc = _hip.LangevinChains(2, 3)
    with pytest.raises(ValueError, match="components"):
        lc.set_mixture(np.zeros((65, 3)), np.ones(65))
    with pytest.raises(ValueError, match="weights"):
        lc.set_mixture(np.zeros((2, 3)), [1.0, -1.0])
    with pytest.raises(ValueError, match="sigma"):
        lc.set_mixture(np.zeros((2, 3)), [1.0, 1.0], [1.0, 0.0])
    with pytest.raises(ValueError, match="eps"):
        lc.set_mixture(np.zeros((2, 3)), [1.0, 1.0], 1.0, -1.0)
    with pytest.raises(ValueError, match="not finite"):
        lc.set_mixture(np.array([[0.0, np.nan, 0.0]]), [1.0])
    lc.close()
    big = _hip.LangevinChains(1, 65537)
    with pytest.raises(ValueError, match="65536"):
        big.set_mixture(np.zeros((1, 65537)), [1.0])
    big.close()

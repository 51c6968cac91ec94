"""K6 Swendsen-Wang on the host: the NumPy twin (tests/helpers/cluster_twin.py) against the oracle's Philox and against exact
enumeration of small lattices, the library's bond threshold, and the Python layer's refusals (no GPU needed)."""
import importlib.util
import math
import os

import numpy as np
import pytest
from scipy.stats import chi2

from oracle import oracle as ora

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("cluster_twin", os.path.join(HERE, "helpers", "cluster_twin.py"))
twin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(twin)


def test_twin_philox_matches_oracle():
    rng = np.random.default_rng(3)
    ctrs = np.concatenate([rng.integers(0, 2 ** 32, size=(60, 4), dtype=np.uint64),
                           np.array([[0, 0, 0, 0], [2 ** 32 - 1] * 4, [1, 2, 3, 6], [5, 7, 11, 7 | (3 << 8)]], np.uint64)])
    for key in ((0, 0), (0xDEADBEEF, 0x12345678), (2 ** 32 - 1, 1)):
        got = twin.philox4x32_10(ctrs[:, 0], ctrs[:, 1], ctrs[:, 2], ctrs[:, 3], *key)
        for i, c in enumerate(ctrs):
            want = ora.philox4x32_10(c.astype(np.uint32), np.array(key, np.uint32))
            assert [int(g[i]) for g in got] == [int(x) for x in want]


def test_cluster_threshold_is_pure_host_code():
    from tsu import _hip
    for J, T in ((1.0, 2.269185), (1.0, 1.5), (-1.0, 3.5), (0.5, 0.7), (2.0, 100.0), (-0.3, 1e-3)):
        p = -math.expm1(-2.0 * abs(J) / T)
        assert _hip.cluster_threshold(J, T) == math.floor(p * 2.0 ** 32) == twin.threshold(J, T)
    assert _hip.cluster_threshold(1.0, 1e-300) == 2 ** 32      # T -> 0: every satisfied bond is active
    assert _hip.cluster_threshold(-1.0, 1e-300) == 2 ** 32
    assert _hip.cluster_threshold(0.0, 1.0) == 0                # J = 0: no bonds
    assert _hip.cluster_threshold(-1.0, 2.0) == _hip.cluster_threshold(1.0, 2.0)
    for T in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            _hip.cluster_threshold(1.0, T)


def _exact_energy_pmf(rows, cols, periodic, J, T):
    n = rows * cols
    states = ((np.arange(2 ** n)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.int64) * 2 - 1
    s = states.reshape(-1, rows, cols)
    if periodic:
        b = np.sum(s * np.roll(s, -1, 2), axis=(1, 2)) + np.sum(s * np.roll(s, -1, 1), axis=(1, 2))
    else:
        b = np.sum(s[:, :, :-1] * s[:, :, 1:], axis=(1, 2)) + np.sum(s[:, :-1, :] * s[:, 1:, :], axis=(1, 2))
    levels, counts = np.unique(b, return_counts=True)
    logw = np.log(counts) + J * levels / T
    w = np.exp(logw - logw.max())
    return levels, w / w.sum()


@pytest.mark.parametrize("rows,cols,periodic,J,T", [
    (4, 4, True, 1.0, 1.5), (4, 4, True, 1.0, 2.269), (4, 4, True, 1.0, 3.5),
    (3, 5, False, 1.0, 2.269), (4, 4, True, -1.0, 2.0),
])
def test_twin_samples_the_boltzmann_energy_distribution(rows, cols, periodic, J, T):
    """20000 twin steps from a random start; the histogram of the bond sum against exact enumeration by a chi^2 test (bins
    with fewer than 5 expected counts merged).  Fixed seed: the outcome is deterministic."""
    n_steps = 20000
    levels, pmf = _exact_energy_pmf(rows, cols, periodic, J, T)
    rng = np.random.default_rng(1)
    s = rng.choice(np.array([-1, 1], np.int8), size=(rows, cols))
    seen = np.empty(n_steps, np.int64)
    for t in range(n_steps):
        s = twin.step(s, periodic, J, T, seed=12345, t=t)
        seen[t] = twin.bond_sum(s, periodic)
    assert set(np.unique(seen)) <= set(levels.tolist())
    observed = np.array([np.sum(seen == v) for v in levels], float)
    expected = pmf * n_steps
    # merge sparse bins into their neighbours, from the rare end inwards
    obs_m, exp_m, o_acc, e_acc = [], [], 0.0, 0.0
    for o, e in zip(observed, expected):
        o_acc += o
        e_acc += e
        if e_acc >= 5:
            obs_m.append(o_acc)
            exp_m.append(e_acc)
            o_acc = e_acc = 0.0
    if e_acc > 0:
        obs_m[-1] += o_acc
        exp_m[-1] += e_acc
    obs_m, exp_m = np.array(obs_m), np.array(exp_m)
    stat = float(np.sum((obs_m - exp_m) ** 2 / exp_m))
    dof = len(obs_m) - 1
    # successive SW states are weakly correlated at these sizes (tau_int of E ~ 1-2 steps): allow a factor 4 on chi^2
    assert chi2.sf(stat / 4.0, dof) > 1e-3, (stat, dof, obs_m, exp_m)
    # and a plain sanity check of the mean energy
    mean_exact = float(np.sum(levels * pmf))
    assert abs(seen.mean() - mean_exact) < 0.1 * max(1.0, abs(mean_exact)), (seen.mean(), mean_exact)


def test_twin_labels_are_min_index_roots_and_respect_boundaries():
    rng = np.random.default_rng(7)
    s = rng.choice(np.array([-1, 1], np.int8), size=(6, 9))
    roots, act_r, act_d = twin.labels(s, False, 1.0, 1e-9, seed=3, t=0)   # T -> 0: every equal-spin bond is active
    assert not act_r[:, -1].any() and not act_d[-1, :].any()
    idx = np.arange(54).reshape(6, 9)
    assert (roots <= idx).all() and (roots[np.unravel_index(roots.ravel(), s.shape)].ravel() == roots.ravel()).all()
    # every root is the smallest index of its cluster and clusters are single-signed
    for r in np.unique(roots):
        members = idx[roots == r]
        assert members.min() == r
        assert len(set(s.ravel()[members].tolist())) == 1
    roots0, act_r0, act_d0 = twin.labels(s, True, 0.0, 1.0, seed=3, t=0)  # J = 0: no bonds
    assert (roots0 == idx).all() and not act_r0.any() and not act_d0.any()


def test_cluster_validation_before_the_device():
    from tsu import _hip
    from tsu.models import ising

    def fake(external_field=0.0, bias_mode="physical"):
        m = ising.IsingModel2D.__new__(ising.IsingModel2D)
        m.external_field, m.bias_mode, m.coupling, m.temperature = external_field, bias_mode, 1.0, 2.0
        m.seed, m.cluster_count, m.sweep_count, m._lat = 1, 0, 0, None  # any device access would raise AttributeError
        return m

    with pytest.raises(_hip.UnsupportedError, match="external_field"):
        fake(external_field=0.5).cluster_update(1)
    with pytest.raises(_hip.UnsupportedError, match="physical"):
        fake(bias_mode="compat").cluster_update(1)
    with pytest.raises(_hip.UnsupportedError, match="external_field"):
        fake(external_field=-1.0).equilibrate(n_sweeps=3, algorithm="swendsen_wang")
    with pytest.raises(ValueError, match="algorithm"):
        fake().equilibrate(n_sweeps=3, algorithm="wolff")
    with pytest.raises(ValueError, match="algorithm"):
        ising.temperature_scan(16, [2.0], algorithm="metropolis")
    with pytest.raises(_hip.UnsupportedError, match="physical"):
        ising.temperature_scan(16, [2.0], bias_mode="compat", algorithm="swendsen_wang")

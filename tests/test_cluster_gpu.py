"""K6 Swendsen-Wang cluster steps on the GPU (csrc/ising2d_cluster.hip): bit-exact against the NumPy twin
(tests/helpers/cluster_twin.py) on both routes and any tile edge, the launch counts of the routes, interleaving with heat-bath
sweeps, the batched temperature scan, Onsager / Yang at 512^2 and the decorrelation at T_c against heat-bath sweeps."""
import importlib.util
import math
import os

import numpy as np
import pytest

from oracle import oracle as ora

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("cluster_twin", os.path.join(HERE, "helpers", "cluster_twin.py"))
twin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(twin)

TC = 2.0 / math.log(1.0 + math.sqrt(2.0))


@pytest.fixture(scope="module")
def hip():
    from tsu import _hip
    return _hip


def _check_calls(hip, rows, cols, periodic, J, T, calls, seed=77, replica=0):
    """Random start, then `calls` = [(step0, n_steps), ...]; every call compared with the twin bit for bit."""
    lat = hip.Lattice(rows, cols, periodic)
    try:
        lat.randomize(seed + 1)
        want = lat.get_spins()
        for step0, n in calls:
            lat.cluster_sweep(J, T, n, seed, step0, replica)
            want = twin.sweep(want, periodic, J, T, n, seed, step0, replica)
            got = lat.get_spins()
            assert (got == want).all(), f"{rows}x{cols} periodic={periodic} J={J} T={T}: step0={step0} differs " \
                                        f"at {np.argwhere(got != want)[:5].tolist()}"
        return want
    finally:
        lat.close()


SMALL_SHAPES = [(4, 4, True), (16, 16, True), (64, 64, True), (128, 128, True),
                (1, 300, False), (300, 1, False), (37, 53, False), (130, 70, False)]


@pytest.mark.parametrize("rows,cols,periodic", SMALL_SHAPES)
@pytest.mark.parametrize("T", [1.5, 2.269, 5.0])
def test_bit_exact_small_lattices(hip, rows, cols, periodic, T):
    _check_calls(hip, rows, cols, periodic, 1.0, T, [(5, 3), (8, 2), (1000, 4)])


@pytest.mark.parametrize("rows,cols,periodic", [(16, 16, True), (37, 53, False), (130, 70, False), (1, 300, False)])
@pytest.mark.parametrize("J", [-1.0, 0.0])
def test_bit_exact_antiferromagnet_and_free_spins(hip, rows, cols, periodic, J):
    _check_calls(hip, rows, cols, periodic, J, 2.0, [(3, 3), (6, 2)], replica=2)


@pytest.mark.parametrize("rows,cols,T", [(256, 512, 1.5), (256, 512, 2.269), (256, 512, 5.0), (1024, 1024, 1.5),
                                         (1024, 1024, 2.269)])
def test_bit_exact_large_lattices(hip, rows, cols, T):
    _check_calls(hip, rows, cols, True, 1.0, T, [(11, 2), (13, 1)])


def test_bit_exact_large_antiferromagnet(hip):
    _check_calls(hip, 256, 512, True, -1.0, 2.0, [(4, 2)])


def test_percolating_cluster_wraps_both_ways(hip):
    """At T = 1.5 from an ordered start the largest cluster spans the periodic lattice in both directions (exercises wrap
    bonds of the merge pass); the GPU agrees with the twin there."""
    lat = hip.Lattice(256, 512, True)
    try:
        lat.fill(1)
        lat.cluster_sweep(1.0, 1.5, 2, 9, 0)
        want = twin.sweep(np.ones((256, 512), np.int8), True, 1.0, 1.5, 2, 9, 0)
        assert (lat.get_spins() == want).all()
        roots, act_r, act_d = twin.labels(want, True, 1.0, 1.5, 9, 2)
        big = np.bincount(roots.ravel()).argmax()
        assert (roots[:, 0] == big).any() and (act_r[:, -1] & (roots[:, -1] == big)).any()
        assert (act_d[-1, :] & (roots[-1, :] == big)).any()
    finally:
        lat.close()


@pytest.mark.parametrize("rows,cols,periodic", [(37, 53, False), (100, 70, True), (130, 70, False), (1, 300, False),
                                                (300, 1, False)])
def test_same_spins_for_every_tile_edge(hip, monkeypatch, rows, cols, periodic):
    outs = []
    for edge in (None, 8, 16, 32):
        if edge is None:
            monkeypatch.delenv("TSU_SW_TILE", raising=False)
        else:
            monkeypatch.setenv("TSU_SW_TILE", str(edge))
        outs.append(_check_calls(hip, rows, cols, periodic, 1.0, 2.269, [(2, 3), (40, 2)]))
    monkeypatch.delenv("TSU_SW_TILE", raising=False)
    for o in outs[1:]:
        assert (o == outs[0]).all()


def test_routes_by_launch_count(hip, monkeypatch):
    monkeypatch.delenv("TSU_SW_TILE", raising=False)
    small = hip.Lattice(64, 64, True)
    small.randomize(1)
    small.cluster_sweep(1.0, 2.269, 1, 5, 0)
    assert small.cluster_launch_count() == 1
    small.cluster_sweep(1.0, 2.269, 25, 5, 1)
    assert small.cluster_launch_count() == 2          # one launch per call, whatever n_steps is
    assert small.launch_count() == 0                  # the sweep-kernel count is not touched
    small.close()
    # a batch of 8 small lattices of one shape: ONE launch (every lattice of it counts that one launch), same spins as serial
    lats = [hip.Lattice(48, 40, False) for _ in range(8)]
    Ts = np.linspace(1.5, 3.5, 8)
    for i, l in enumerate(lats):
        l.randomize(100 + i)
    starts = [l.get_spins() for l in lats]
    hip.cluster_sweep_batch(lats, 4, [1.0] * 8, Ts, [7 + i for i in range(8)], [3 * i for i in range(8)], list(range(8)))
    for i, l in enumerate(lats):
        assert l.cluster_launch_count() == 1
        assert (l.get_spins() == twin.sweep(starts[i], False, 1.0, Ts[i], 4, 7 + i, 3 * i, i)).all()
        l.close()
    # a large lattice: a fixed number of launches per step
    big = hip.Lattice(256, 512, True)
    big.randomize(2)
    big.cluster_sweep(1.0, 2.269, 1, 5, 0)
    per_step = big.cluster_launch_count()
    big.cluster_sweep(1.0, 2.269, 7, 5, 1)
    assert per_step == 3 and big.cluster_launch_count() == 8 * per_step
    big.close()


def test_interleaving_with_heat_bath_sweeps(hip):
    from tsu.models.ising import IsingModel2D
    J, T, seed = 1.0, 2.269, 4242
    m = IsingModel2D(size=(32, 48), coupling=J, temperature=T, seed=seed)
    s = ora.ising2d_randomize(32, 48, seed)
    assert (m.spins == s).all()
    table = ora.ising2d_thresholds(J, 0.0, T, ora.MODE_PHYSICAL)
    m.gibbs_update(3)
    s = ora.ising2d_sweep(s, True, table, 3, seed, 0)
    m.cluster_update(4)
    s = twin.sweep(s, True, J, T, 4, seed, 0)
    m.gibbs_update(2)
    s = ora.ising2d_sweep(s, True, table, 2, seed, 3)
    assert m.sweep_count == 5 and m.cluster_count == 4
    assert (m.spins == s).all()
    m.equilibrate(n_sweeps=2, algorithm="swendsen_wang")
    assert (m.spins == twin.sweep(s, True, J, T, 2, seed, 4)).all() and m.cluster_count == 6 and m.sweep_count == 5


def test_temperature_scan_batch_equals_serial(hip):
    from tsu.models.ising import IsingModel2D, temperature_scan
    temps = [1.5, 2.0, 2.269, 3.0]
    out = temperature_scan(32, temps, n_equilibrate=10, n_measure=6, measure_every=3, seed=5, algorithm="swendsen_wang")
    for i, T in enumerate(temps):
        m = IsingModel2D(32, temperature=T, seed=5 + i, initial="up")
        m.cluster_update(10)
        Ms, Es = [], []
        for _ in range(6):
            m.cluster_update(3)
            Ms.append(m.magnetization())
            Es.append(m.energy())
        Ms, Es = np.array(Ms), np.array(Es)
        assert out["magnetization"][i] == np.mean(np.abs(Ms))
        assert out["energy"][i] == np.mean(Es) / m.n_spins
        assert out["susceptibility"][i] == (np.mean(Ms ** 2) - np.mean(np.abs(Ms)) ** 2) * m.n_spins / T
        assert out["specific_heat"][i] == (np.mean(Es ** 2) - np.mean(Es) ** 2) / (T ** 2 * m.n_spins)
        assert m.sweep_count == 0


def _onsager_energy(T, J=1.0):
    from scipy.special import ellipk
    b = 1.0 / T
    k = 2.0 * math.sinh(2 * b * J) / math.cosh(2 * b * J) ** 2
    return -J / math.tanh(2 * b * J) * (1 + 2 / math.pi * (2 * math.tanh(2 * b * J) ** 2 - 1) * ellipk(k * k))


@pytest.mark.parametrize("T", [2.0, 3.0])
def test_onsager_and_yang_at_512(hip, T):
    from tsu.models.ising import IsingModel2D
    m = IsingModel2D(512, temperature=T, seed=31, initial="up")
    m.cluster_update(200)
    n_batches, per = 20, 100
    E, M = np.zeros((n_batches, per)), np.zeros((n_batches, per))
    for b in range(n_batches):
        for j in range(per):
            m.cluster_update(1)
            E[b, j] = m.energy() / m.n_spins
            M[b, j] = abs(m.magnetization())
    e_b, m_b = E.mean(axis=1), M.mean(axis=1)
    e_se, m_se = e_b.std(ddof=1) / math.sqrt(n_batches), m_b.std(ddof=1) / math.sqrt(n_batches)
    e_exact = _onsager_energy(T)
    assert abs(e_b.mean() - e_exact) < 4 * e_se, (e_b.mean(), e_exact, e_se)
    if T < TC:
        m_exact = (1 - math.sinh(2 / T) ** -4) ** 0.125
        assert abs(m_b.mean() - m_exact) < 4 * m_se, (m_b.mean(), m_exact, m_se)


def _tau_int(x, c=6.0):
    """integrated autocorrelation time with Sokal's automatic window"""
    x = np.asarray(x, float) - np.mean(x)
    n = len(x)
    f = np.fft.rfft(x, 2 * n)
    acf = np.fft.irfft(f * np.conj(f))[:n]
    acf /= acf[0]
    tau = 0.5
    for w in range(1, n):
        tau += acf[w]
        if w >= c * tau:
            break
    return tau


def test_cluster_steps_decorrelate_faster_than_heat_bath_at_tc(hip):
    from tsu.models.ising import IsingModel2D
    m = IsingModel2D(64, temperature=TC, seed=17)
    m.cluster_update(1000)
    n = 20000
    sw = np.empty(n)
    for i in range(n):
        m.cluster_update(1)
        sw[i] = abs(m.magnetization())
    every = 4
    hb = np.empty(n)
    for i in range(n):
        m.gibbs_update(every)
        hb[i] = abs(m.magnetization())
    tau_sw, tau_hb = _tau_int(sw), every * _tau_int(hb)
    print(f"\n64^2 at T_c: tau_int(|m|) SW {tau_sw:.2f} steps, heat-bath {tau_hb:.1f} sweeps, ratio {tau_hb / tau_sw:.1f}")
    assert tau_hb >= 10 * tau_sw, (tau_sw, tau_hb)


def test_errors(hip):
    slab = hip.Lattice(32, 64, True, total_rows=64, row0=0, ghost=2)
    with pytest.raises(hip.UnsupportedError):
        slab.cluster_sweep(1.0, 2.0, 1, 1, 0)
    slab.close()
    lat = hip.Lattice(16, 16, True)
    for T in (0.0, -1.0):
        with pytest.raises(ValueError):
            lat.cluster_sweep(1.0, T, 1, 1, 0)
        with pytest.raises(ValueError):
            hip.cluster_sweep_batch([lat], 1, [1.0], [T], [1], [0])
    lat.cluster_sweep(1.0, 2.0, 0, 1, 0)
    assert lat.cluster_launch_count() == 0
    lat.close()

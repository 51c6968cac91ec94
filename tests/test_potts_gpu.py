"""K10, the q-state Potts lattice, on the GPU (csrc/potts2d.hip): heat-bath sweeps and Swendsen-Wang steps bit for bit against the
NumPy twin (tests/helpers/potts_twin.py) on every route, the integer observables and the recorded runs, exact enumeration on the
device, the two algorithms against each other, and q = 2 against IsingModel2D."""
import importlib.util
import itertools
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


pt = _load("potts_twin")


@pytest.fixture(scope="module")
def hip():
    from tsu import _hip
    return _hip


# (rows, cols, periodic): 2x2, one row, one column; a small periodic lattice; the double bond with a width that is no multiple of the
# 16 columns of a Philox block; odd widths; the last k10_small lattice; the first native k10_sweep lattice; a wide open one
# k10_sweep reads rows of whole octets (cols % 16 == 0) by 16-byte loads: one periodic octet that wraps onto itself, and an open
# lattice of two octets a row with an odd number of rows
SHAPES = [(2, 2, False), (1, 7, False), (7, 1, False), (6, 10, True), (2, 18, True), (33, 65, False), (128, 128, True),
          (130, 128, True), (70, 258, False), (4, 16, True), (5, 32, False)]
SEEDS = (2 ** 64 - 59, 0x9E3779B97F4A7C15, 12345)
FIELDS = {2: (0.0, 0.25), 3: (0.3, 0.0, -0.2), 5: (0.1, -0.3, 0.2, 0.0, 0.4), 8: (0.5, -0.5, 0.25, 0.0, -0.25, 0.1, -0.1, 0.3)}
TEMPS = (0.2, 0.7, 1.0, 2.0, 5.0)


def _models():
    """q x J x (with and without h), with T, replica, sweep0 and the seed cycling through their values."""
    out = []
    for i, (q, J, with_h) in enumerate(itertools.product((2, 3, 5, 8), (1.0, -1.0, 0.37), (False, True))):
        out.append(dict(q=q, J=J, h=FIELDS[q] if with_h else None, T=TEMPS[i % len(TEMPS)], replica=(0, 3)[(i // 2) % 2],
                        sweep0=(0, 2 ** 32 - 4)[(i // 3) % 2], seed=SEEDS[i % len(SEEDS)]))
    return out


def _check_measure(lat, s, q, periodic):
    n_eq, N = lat.measure()
    w_eq, w_N = pt.measure(s, q, periodic)
    assert n_eq == w_eq and N.tolist() == w_N.tolist()


@pytest.mark.parametrize("rows,cols,periodic", SHAPES)
def test_heat_bath_equals_the_twin_on_both_routes(hip, monkeypatch, rows, cols, periodic):
    """6 sweeps from a random start; then a call of 3 sweeps against 3 calls of one; n_eq and N_c on every state."""
    small = rows * cols <= 16384
    models = _models()
    if rows * cols > 4096:  # the large lattices take every q, J and h once each way, not the full product
        models = models[::5]
    rng = np.random.default_rng(rows * 1000 + cols)
    for m in models:
        q = m["q"]
        start = rng.integers(0, q, size=(rows, cols)).astype(np.int8)
        want = pt.sweep(start, q, periodic, m["J"], m["h"], m["T"], 6, m["seed"], m["sweep0"], m["replica"])
        for route in (("k10_small", "k10_sweep") if small else ("k10_sweep",)):
            if small and route == "k10_sweep":
                monkeypatch.setenv("TSU_POTTS_SMALL", "0")
            else:
                monkeypatch.delenv("TSU_POTTS_SMALL", raising=False)
            lat = hip.PottsLattice(rows, cols, q, periodic)
            try:
                assert lat.route() == route
                lat.set_model(m["J"], m["h"])
                lat.set_spins(start)
                n0 = lat.launch_count()
                lat.sweep(m["T"], 6, m["seed"], m["sweep0"], m["replica"])
                assert lat.launch_count() - n0 == (1 if route == "k10_small" else 12)
                got = lat.get_spins()
                assert (got == want).all(), f"{m} {route}: differs at {np.argwhere(got != want)[:5].tolist()}"
                _check_measure(lat, want, q, periodic)
                # a call of n sweeps equals n calls of one sweep (the counter wraps through 2^32 where sweep0 is at the top)
                lat.sweep(m["T"], 3, m["seed"], (m["sweep0"] + 6) % 2 ** 32, m["replica"])
                one = lat.get_spins()
                lat.set_spins(want)
                for k in range(3):
                    lat.sweep(m["T"], 1, m["seed"], (m["sweep0"] + 6 + k) % 2 ** 32, m["replica"])
                assert (lat.get_spins() == one).all()
            finally:
                lat.close()
        monkeypatch.delenv("TSU_POTTS_SMALL", raising=False)


def _tc(q):
    return 1.0 / math.log(1.0 + math.sqrt(q))


@pytest.mark.parametrize("rows,cols,periodic", SHAPES)
def test_cluster_steps_equal_the_twin_on_every_route(hip, monkeypatch, rows, cols, periodic):
    """k10_sw_small, the tiled route where it is native (130 x 128, 70 x 258) and forced with TSU_SW_TILE = 4, 6 and 64 (seams,
    wraps and a narrow last tile); the step counters split over two calls; n_eq and N_c on every state."""
    native = "k10_sw_small" if rows * cols <= 16384 else "k10_sw_tiles"
    rng = np.random.default_rng(rows * 1000 + cols + 1)
    for i, (q, fac) in enumerate(itertools.product((2, 3, 8), (0.8, 1.0, 1.3))):
        T = fac * _tc(q)
        J, seed, replica = (1.0, 0.37, 2.5)[i % 3], SEEDS[i % 3], (0, 3)[i % 2]
        T *= J
        step0 = (5, 2 ** 32 - 6)[i % 2]
        start = rng.integers(0, q, size=(rows, cols)).astype(np.int8)
        mid = pt.cluster_sweep(start, q, periodic, J, T, 2, seed, step0, replica)
        want = pt.cluster_sweep(mid, q, periodic, J, T, 4, seed, step0 + 2, replica)
        tiles = (None, "4", "6", "64") if rows * cols <= 4096 or fac == 1.0 else (None, "64")
        for tile in tiles:
            if tile is None:
                monkeypatch.delenv("TSU_SW_TILE", raising=False)
            else:
                monkeypatch.setenv("TSU_SW_TILE", tile)
            lat = hip.PottsLattice(rows, cols, q, periodic)
            try:
                assert lat.route(hip.POTTS_SWENDSEN_WANG) == (native if tile is None else "k10_sw_tiles")
                lat.set_model(J)
                lat.set_spins(start)
                lat.cluster_sweep(T, 2, seed, step0, replica)
                got = lat.get_spins()
                assert (got == mid).all(), f"q={q} T={T} tile={tile}: differs at {np.argwhere(got != mid)[:5].tolist()}"
                _check_measure(lat, mid, q, periodic)
                lat.cluster_sweep(T, 4, seed, step0 + 2, replica)
                got = lat.get_spins()
                assert (got == want).all(), f"q={q} T={T} tile={tile}: differs at {np.argwhere(got != want)[:5].tolist()}"
                _check_measure(lat, want, q, periodic)
            finally:
                lat.close()
        monkeypatch.delenv("TSU_SW_TILE", raising=False)


def test_cluster_steps_refuse_an_antiferromagnet_and_a_field(hip):
    rng = np.random.default_rng(4)
    start = rng.integers(0, 3, size=(6, 10)).astype(np.int8)
    for J, h in ((-1.0, None), (0.0, None), (1.0, (0.0, 0.1, 0.0))):
        lat = hip.PottsLattice(6, 10, 3, True)
        try:
            lat.set_model(J, h)
            lat.set_spins(start)
            n0 = lat.launch_count()
            with pytest.raises(hip.UnsupportedError):
                lat.cluster_sweep(1.0, 2, 5)
            with pytest.raises(hip.UnsupportedError):
                lat.run(1.0, 2, 1, hip.POTTS_SWENDSEN_WANG, 5)
            assert lat.launch_count() == n0 and (lat.get_spins() == start).all()
            lat.sweep(1.0, 1, 5)  # heat-bath sweeps take the same model
        finally:
            lat.close()
    lat = hip.PottsLattice(6, 10, 3, True)
    try:
        with pytest.raises(ValueError):
            lat.set_spins(np.full((6, 10), 3, np.int8))
        with pytest.raises(ValueError):
            lat.set_spins(np.full((6, 10), -1, np.int8))
        with pytest.raises(ValueError):
            lat.sweep(0.001, 1, 5)  # 4 |J| / T > 600
        with pytest.raises(ValueError):
            lat.cluster_sweep(1.0, 8, 5, step0=2 ** 32 - 4)
        assert (lat.get_spins() == 0).all()
    finally:
        lat.close()


@pytest.mark.parametrize("rows,cols,periodic,q", [(6, 10, True, 3), (33, 65, False, 8), (130, 128, True, 5)])
@pytest.mark.parametrize("algorithm", ["heat_bath", "swendsen_wang"])
def test_run_rows_equal_the_handle_step_by_step(hip, rows, cols, periodic, q, algorithm):
    """tsu_potts2d_run against single calls with a measurement after each, row for row; a run split in two equals one run; the
    launch count is that of the updates plus one measurement a row, so nothing came back to the host in between."""
    alg = hip.POTTS_HEAT_BATH if algorithm == "heat_bath" else hip.POTTS_SWENDSEN_WANG
    T, seed, c0, every, n_meas = 1.1 * _tc(q), SEEDS[1], 7, 3, 6
    start = np.random.default_rng(9).integers(0, q, size=(rows, cols)).astype(np.int8)
    a, b, c = (hip.PottsLattice(rows, cols, q, periodic) for _ in range(3))
    try:
        for lat in (a, b, c):
            lat.set_spins(start)
        n0 = a.launch_count()
        a.run(T, n_meas, every, alg, seed, c0, 2)
        per_update = {"k10_small": 1, "k10_sweep": 2 * every, "k10_sw_small": 1, "k10_sw_tiles": 3 * every}[a.route(alg)]
        assert a.launch_count() - n0 == n_meas * (per_update + 1)
        rows_a = a.record()
        assert rows_a.shape == (n_meas, 9) and (rows_a[:, 1 + q:] == 0).all()
        for k in range(n_meas):
            if alg == hip.POTTS_HEAT_BATH:
                b.sweep(T, every, seed, c0 + k * every, 2)
            else:
                b.cluster_sweep(T, every, seed, c0 + k * every, 2)
            n_eq, N = b.measure()
            assert rows_a[k, 0] == n_eq and rows_a[k, 1:1 + q].tolist() == N.tolist(), k
            w_eq, w_N = pt.measure(b.get_spins(), q, periodic)
            assert n_eq == w_eq and N.tolist() == w_N.tolist()
        assert (a.get_spins() == b.get_spins()).all()
        c.run(T, 2, every, alg, seed, c0, 2)
        first = c.record()
        c.run(T, n_meas - 2, every, alg, seed, c0 + 2 * every, 2)
        assert (np.concatenate([first, c.record()]) == rows_a).all() and (c.get_spins() == a.get_spins()).all()
    finally:
        for lat in (a, b, c):
            lat.close()


def _device_codes(lat, q, update, n_discard, n_states, every):
    update(n_discard, 0)
    codes = []
    for k in range(n_states):
        update(every, n_discard + k * every)
        codes.append(pt.state_code(lat.get_spins(), q))
    return codes


@pytest.mark.parametrize("case", pt.ENUMERATION_HEAT_BATH[:3], ids=lambda c: f"{c[0][0]}x{c[0][1]}-q{c[1]}")
def test_heat_bath_enumeration_on_the_device(hip, case):
    """The CPU test's chains on the device: the first 50 recorded states equal the twin's, and the 20 000 states pass the same
    chi^2 check.  The twin gives, and the device gave on an MI355X, digit for digit:
      open 2x3 q=3 J=1  T=1.5 h=(0.3, 0, -0.2): chi2 = 689.8 on 665 dof, p = 0.245, pooled 1.2 %
      open 2x2 q=5 J=1  T=1.2 h=0:              chi2 = 597.3 on 624 dof, p = 0.772, pooled 0 %
      open 3x3 q=2 J=-1 T=1.0 h=(0, 0.25):      chi2 = 315.1 on 330 dof, p = 0.713, pooled 1.6 %"""
    shape, q, J, T, h, seed = case
    lat = hip.PottsLattice(shape[0], shape[1], q, False)
    try:
        lat.set_model(J, h)
        codes = _device_codes(lat, q, lambda n, c0: lat.sweep(T, n, seed, c0), 100, 20000, 4)
    finally:
        lat.close()
    s, _ = pt.chain(np.zeros(shape, np.int8), q, False, J, h, T, 100, seed)
    _, want = pt.chain(s, q, False, J, h, T, 200, seed, sweep0=100, record_every=4)
    assert codes[:50] == want
    chi2, dof, p, pooled = pt.boltzmann_chi2(codes, shape, q, False, J, h, T)
    print(f"\n{shape} q={q}: chi2 = {chi2:.1f} on {dof} dof, p = {p:.3f}, pooled {100 * pooled:.1f} %")
    assert p >= 0.01 and pooled <= 0.05


@pytest.mark.parametrize("case", pt.ENUMERATION_CLUSTER, ids=lambda c: f"{c[0][0]}x{c[0][1]}-q{c[1]}")
def test_cluster_enumeration_on_the_device(hip, case):
    """The same for Swendsen-Wang steps.  The twin gives, and the device gave:
      open 2x3 q=3 J=1 T=1.5: chi2 = 699.1 on 675 dof, p = 0.253, pooled 1.1 %
      open 2x2 q=5 J=1 T=1.2: chi2 = 646.7 on 624 dof, p = 0.257, pooled 0 %"""
    shape, q, J, T, seed = case
    lat = hip.PottsLattice(shape[0], shape[1], q, False)
    try:
        lat.set_model(J)
        codes = _device_codes(lat, q, lambda n, c0: lat.cluster_sweep(T, n, seed, c0), 100, 20000, 4)
    finally:
        lat.close()
    s, _ = pt.cluster_chain(np.zeros(shape, np.int8), q, False, J, T, 100, seed)
    _, want = pt.cluster_chain(s, q, False, J, T, 200, seed, step0=100, record_every=4)
    assert codes[:50] == want
    chi2, dof, p, pooled = pt.boltzmann_chi2(codes, shape, q, False, J, None, T)
    print(f"\n{shape} q={q}: chi2 = {chi2:.1f} on {dof} dof, p = {p:.3f}, pooled {100 * pooled:.1f} %")
    assert p >= 0.01 and pooled <= 0.05


def _batch_means(x, n_batches=20):
    x = np.asarray(x, dtype=np.float64)
    b = x[: len(x) // n_batches * n_batches].reshape(n_batches, -1).mean(axis=1)
    return float(x.mean()), float(b.std(ddof=1) / math.sqrt(n_batches))


@pytest.mark.parametrize("factor", [0.9, 1.1])
def test_heat_bath_and_cluster_steps_agree_at_q3(factor):
    """32 x 32 periodic, q = 3, T = factor T_c: <e> and <m> of the two algorithms within 4 combined batch-means errors.  Run lengths
    from the twin (6000 sweeps / 3000 steps at the same size): tau_int of (e, m) is (2.5, 4.0) sweeps and (3.3, 3.1) steps at
    0.9 T_c, (4.1, 13.3) sweeps and (3.1, 0.9) steps at 1.1 T_c.  Here: 500 updates discarded, then 4000 measurements 5 sweeps
    (2 steps) apart in 20 batches: a batch is 1000 sweeps (400 steps), 75 (120) times the longest tau_int."""
    import tsu
    T = factor * _tc(3)
    res = {}
    for algorithm, every in (("heat_bath", 5), ("swendsen_wang", 2)):
        model = tsu.PottsModel2D(32, 3, temperature=T, seed=21)
        model.equilibrate(n_sweeps=500, algorithm=algorithm)
        rows = model.run(4000, every, algorithm)
        model.close()
        res[algorithm] = (_batch_means(-rows[:, 0] / 1024.0), _batch_means(pt.order_parameter(rows[:, 1:], 3)))
    for k, name in enumerate(("e", "m")):
        (a, ea), (b, eb) = res["heat_bath"][k], res["swendsen_wang"][k]
        print(f"\n{factor} T_c <{name}>: heat bath {a:.5f} +- {ea:.5f}, cluster {b:.5f} +- {eb:.5f}")
        assert abs(a - b) <= 4.0 * math.hypot(ea, eb)


@pytest.mark.parametrize("T", [2.0, 2.5])
def test_q2_agrees_with_the_ising_model(T):
    """q = 2 is the Ising model under J_Potts = 2 J_Ising: at 16 x 16, <n_eq> agrees with (N_b - E_Ising / J) / 2 of IsingModel2D
    within 4 combined batch-means errors (500 sweeps discarded, 2000 measurements 5 sweeps apart, 20 batches of 500 sweeps)."""
    import tsu
    n_b = 2 * 256
    potts = tsu.PottsModel2D(16, 2, temperature=T, coupling=2.0, seed=31)
    potts.equilibrate(n_sweeps=500)
    rows = potts.run(2000, 5)
    potts.close()
    ising = tsu.IsingModel2D(size=16, coupling=1.0, temperature=T, seed=32)
    ising.gibbs_update(500)
    x = []
    for _ in range(2000):
        ising.gibbs_update(5)
        x.append((n_b - ising.energy() / 1.0) / 2.0)
    (a, ea), (b, eb) = _batch_means(rows[:, 0]), _batch_means(x)
    print(f"\nT = {T}: <n_eq> Potts {a:.3f} +- {ea:.3f}, Ising {b:.3f} +- {eb:.3f}")
    assert abs(a - b) <= 4.0 * math.hypot(ea, eb)


def test_model_facade_and_scan():
    import tsu
    m = tsu.PottsModel2D((6, 10), 3, temperature=1.0, field=(0.1, 0.0, -0.1), seed=5)
    start = np.random.default_rng(5).integers(0, 3, size=(6, 10)).astype(np.int8)
    assert (m.spins == start).all() and m.route() == "k10_small" and m.route("swendsen_wang") == "k10_sw_small"
    m.gibbs_update(2).gibbs_update(1)
    want = pt.sweep(start, 3, True, 1.0, (0.1, 0.0, -0.1), 1.0, 3, 5)
    assert (m.spins == want).all() and m.sweep_count == 3
    assert m.energy() == pt.energy(want, 3, True, 1.0, (0.1, 0.0, -0.1))
    assert m.colour_counts().tolist() == pt.measure(want, 3, True)[1].tolist()
    assert m.order_parameter() == pt.order_parameter(pt.measure(want, 3, True)[1], 3)
    with pytest.raises(tsu._hip.UnsupportedError):
        m.cluster_update()
    with pytest.raises(ValueError):
        m.spins = np.full((6, 10), 3)
    m.spins = np.ones((6, 10), np.int64)
    assert (m.fill(2).spins == 2).all() and m.launch_count() >= 2
    m.close()
    res = tsu.potts_temperature_scan(8, 3, [0.5, 3.0], n_equilibrate=200, n_measure=100, measure_every=2, algorithm="swendsen_wang", seed=3)
    assert res["order_parameter"][0] > 0.9 > 0.5 > res["order_parameter"][1] and res["energy"][0] < res["energy"][1]
    assert all(res[k].shape == (2,) for k in ("specific_heat", "susceptibility", "binder"))

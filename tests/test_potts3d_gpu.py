"""K10 on the cubic lattice, on the GPU (csrc/potts3d.hip): heat-bath sweeps and Swendsen-Wang steps bit for bit against the NumPy
twin (tests/helpers/potts3d_twin.py) on every route and tile shape, one layer against the 2-D handle, the integer observables and
the recorded runs, exact enumeration on the device, the two algorithms against each other at q = 3, and q = 2 against IsingModel3D."""
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


p3 = _load("potts3d_twin")
OPEN, ALL = p3.OPEN, p3.ALL


@pytest.fixture(scope="module")
def hip():
    from tsu import _hip
    return _hip


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in ("TSU_POTTS_SMALL", "TSU_SW3D_TILE", "TSU_SW_TILE"):
        monkeypatch.delenv(name, raising=False)


# (depth, rows, cols, periodic): the smallest cube, open and with double bonds on three axes; one layer; a column along z; odd sizes;
# a width that is no multiple of 16; mixed flags; one whole octet wrapping onto itself; whole octets with odd rows; the last small
# lattice; the first native HBM lattice (whole octets); a native HBM lattice on the byte route
SHAPES = [(2, 2, 2, OPEN), (2, 2, 2, ALL), (1, 6, 10, (False, True, True)), (7, 1, 1, OPEN), (3, 5, 7, OPEN), (2, 2, 18, ALL),
          (4, 5, 6, (True, False, True)), (2, 4, 16, ALL), (3, 5, 32, OPEN), (16, 32, 32, ALL), (18, 32, 32, ALL), (5, 70, 66, OPEN)]
SHAPE_IDS = ["x".join(map(str, s[:3])) + "-" + "".join("p" if x else "o" for x in s[3]) for s in SHAPES]
SEEDS = (2 ** 64 - 59, 0x9E3779B97F4A7C15, 12345)
FIELDS = {2: (0.0, 0.25), 3: (0.3, 0.0, -0.2), 5: (0.1, -0.3, 0.2, 0.0, 0.4), 8: (0.5, -0.5, 0.25, 0.0, -0.25, 0.1, -0.1, 0.3)}
TEMPS = (0.2, 0.7, 1.0, 2.0, 5.0)
SMALL_SITES = 16384


def _models():
    """q x J x (with and without h), with T, replica, sweep0 and the seed cycling through their values (the 2-D test's product)."""
    out = []
    for i, (q, J, with_h) in enumerate(itertools.product((2, 3, 5, 8), (1.0, -1.0, 0.37), (False, True))):
        out.append(dict(q=q, J=J, h=FIELDS[q] if with_h else None, T=TEMPS[i % len(TEMPS)], replica=(0, 3)[(i // 2) % 2],
                        sweep0=(0, 2 ** 32 - 4)[(i // 3) % 2], seed=SEEDS[i % len(SEEDS)]))
    return out


def _check_measure(lat, s, q, periodic):
    n_eq, N = lat.measure()
    w_eq, w_N = p3.measure(s, q, periodic)
    assert n_eq == w_eq and N.tolist() == w_N.tolist()


@pytest.mark.parametrize("depth,rows,cols,periodic", SHAPES, ids=SHAPE_IDS)
def test_heat_bath_equals_the_twin_on_both_routes(hip, monkeypatch, depth, rows, cols, periodic):
    """6 sweeps from a random start; then a call of 3 sweeps against 3 calls of one; n_eq and N_c on every state."""
    shape = (depth, rows, cols)
    sites = depth * rows * cols
    small = sites <= SMALL_SITES
    models = _models()
    if sites > 4096:  # the large lattices take every q, J and h once each way, not the full product
        models = models[::5]
    rng = np.random.default_rng(depth * 100000 + rows * 1000 + cols)
    for m in models:
        q = m["q"]
        start = rng.integers(0, q, size=shape).astype(np.int8)
        want = p3.sweep(start, q, periodic, m["J"], m["h"], m["T"], 6, m["seed"], m["sweep0"], m["replica"])
        for route in (("k10_3d_small", "k10_3d_sweep") if small else ("k10_3d_sweep",)):
            if small and route == "k10_3d_sweep":
                monkeypatch.setenv("TSU_POTTS_SMALL", "0")
            else:
                monkeypatch.delenv("TSU_POTTS_SMALL", raising=False)
            lat = hip.PottsLattice3D(depth, rows, cols, q, periodic)
            try:
                assert lat.route() == route
                lat.set_model(m["J"], m["h"])
                lat.set_spins(start)
                n0 = lat.launch_count()
                lat.sweep(m["T"], 6, m["seed"], m["sweep0"], m["replica"])
                assert lat.launch_count() - n0 == (1 if route == "k10_3d_small" else 12)
                got = lat.get_spins()
                assert (got == want).all(), f"{m} {route}: differs at {np.argwhere(got != want)[:5].tolist()}"
                _check_measure(lat, want, q, periodic)
                # a call of n sweeps equals n calls of one sweep (the counter wraps through 2^32 where sweep0 is at the top)
                lat.sweep(m["T"], 3, m["seed"], (m["sweep0"] + 6) % 2 ** 32, m["replica"])
                one = lat.get_spins()
                _check_measure(lat, one, q, periodic)
                lat.set_spins(want)
                for k in range(3):
                    lat.sweep(m["T"], 1, m["seed"], (m["sweep0"] + 6 + k) % 2 ** 32, m["replica"])
                assert (lat.get_spins() == one).all()
            finally:
                lat.close()
        monkeypatch.delenv("TSU_POTTS_SMALL", raising=False)


T_NOMINAL = 1.8  # times J: near the q = 3 transition of the cubic lattice


@pytest.mark.parametrize("depth,rows,cols,periodic", SHAPES, ids=SHAPE_IDS)
def test_cluster_steps_equal_the_twin_on_every_route(hip, monkeypatch, depth, rows, cols, periodic):
    """The native route (k10_3d_sw_small up to 16384 sites, tiles of 8 x 16 x 32 beyond) and the tiled route forced with
    TSU_SW3D_TILE = 2x4x4, 3x5x6 and 8x16x32 (seams and wraps on all three axes, narrow last tiles, a tile larger than the lattice);
    the step counters split over two calls; n_eq and N_c on every state."""
    shape = (depth, rows, cols)
    sites = depth * rows * cols
    native = "k10_3d_sw_small" if sites <= SMALL_SITES else "k10_3d_sw_tiles"
    rng = np.random.default_rng(depth * 100000 + rows * 1000 + cols + 1)
    for i, (q, fac) in enumerate(itertools.product((2, 3, 8), (0.8, 1.0, 1.3))):
        J, seed, replica = (1.0, 0.37, 2.5)[i % 3], SEEDS[i % 3], (0, 3)[i % 2]
        T = fac * T_NOMINAL * J
        step0 = (5, 2 ** 32 - 6)[i % 2]
        start = rng.integers(0, q, size=shape).astype(np.int8)
        mid = p3.cluster_sweep(start, q, periodic, J, T, 2, seed, step0, replica)
        want = p3.cluster_sweep(mid, q, periodic, J, T, 4, seed, step0 + 2, replica)
        tiles = (None, "2x4x4", "3x5x6", "8x16x32") if sites <= 4096 or fac == 1.0 else (None, "8x16x32")
        for tile in tiles:
            if tile is None:
                monkeypatch.delenv("TSU_SW3D_TILE", raising=False)
            else:
                monkeypatch.setenv("TSU_SW3D_TILE", tile)
            lat = hip.PottsLattice3D(depth, rows, cols, q, periodic)
            try:
                assert lat.route(hip.POTTS_SWENDSEN_WANG) == (native if tile is None else "k10_3d_sw_tiles")
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
        monkeypatch.delenv("TSU_SW3D_TILE", raising=False)


@pytest.mark.parametrize("rows,cols,periodic", [(6, 10, True), (2, 18, True), (4, 16, True), (5, 32, False), (33, 65, False)])
def test_one_layer_equals_the_2d_handle(hip, monkeypatch, rows, cols, periodic):
    """PottsLattice3D(1, R, C) with periodic (False, p, p) against PottsLattice(R, C): heat bath on both routes each side, with a
    field and J < 0; cluster steps on the small route and on forced tiles (TSU_SW_TILE for the 2-D handle, TSU_SW3D_TILE for the
    3-D one, read per call)."""
    rng = np.random.default_rng(rows * 1000 + cols + 2)
    per3 = (False, periodic, periodic)
    for q, J, h, T in ((3, 1.0, FIELDS[3], 1.1), (8, -1.0, None, 0.7), (2, 0.37, FIELDS[2], 2.0), (5, -1.0, FIELDS[5], 0.9)):
        start = rng.integers(0, q, size=(rows, cols)).astype(np.int8)
        got = {}
        for dim, small in itertools.product((2, 3), (True, False)):
            if small:
                monkeypatch.delenv("TSU_POTTS_SMALL", raising=False)
            else:
                monkeypatch.setenv("TSU_POTTS_SMALL", "0")
            lat = hip.PottsLattice(rows, cols, q, periodic) if dim == 2 else hip.PottsLattice3D(1, rows, cols, q, per3)
            try:
                assert lat.route() == {2: "k10", 3: "k10_3d"}[dim] + ("_small" if small else "_sweep")
                lat.set_model(J, h)
                lat.set_spins(start)
                lat.sweep(T, 5, SEEDS[0], 2 ** 32 - 3, 3)
                got[dim, small] = (lat.get_spins().reshape(rows, cols), lat.measure())
            finally:
                lat.close()
        monkeypatch.delenv("TSU_POTTS_SMALL", raising=False)
        ref, (ref_eq, ref_N) = got[2, True]
        for key, (s, (n_eq, N)) in got.items():
            assert (s == ref).all() and n_eq == ref_eq and N.tolist() == ref_N.tolist(), (q, key)
    for q, J, T in ((3, 1.0, 1.0), (8, 2.5, 1.9), (2, 0.37, 0.45)):
        start = rng.integers(0, q, size=(rows, cols)).astype(np.int8)
        got = {}
        for dim, tile in itertools.product((2, 3), (None, "4", "6")):
            for name in ("TSU_SW_TILE", "TSU_SW3D_TILE"):
                monkeypatch.delenv(name, raising=False)
            if tile is not None:
                monkeypatch.setenv("TSU_SW_TILE" if dim == 2 else "TSU_SW3D_TILE", tile if dim == 2 else f"1x{tile}x{tile}")
            lat = hip.PottsLattice(rows, cols, q, periodic) if dim == 2 else hip.PottsLattice3D(1, rows, cols, q, per3)
            try:
                assert lat.route(hip.POTTS_SWENDSEN_WANG) == {2: "k10", 3: "k10_3d"}[dim] + ("_sw_small" if tile is None else "_sw_tiles")
                lat.set_model(J)
                lat.set_spins(start)
                lat.cluster_sweep(T, 5, SEEDS[1], 2 ** 32 - 5, 3)
                got[dim, tile] = lat.get_spins().reshape(rows, cols)
            finally:
                lat.close()
        for key, s in got.items():
            assert (s == got[2, None]).all(), (q, key)


def test_cluster_steps_refuse_an_antiferromagnet_and_a_field(hip):
    rng = np.random.default_rng(4)
    start = rng.integers(0, 3, size=(4, 6, 10)).astype(np.int8)
    for J, h in ((-1.0, None), (0.0, None), (1.0, (0.0, 0.1, 0.0))):
        lat = hip.PottsLattice3D(4, 6, 10, 3, True)
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
    lat = hip.PottsLattice3D(4, 6, 10, 3, True)
    try:
        with pytest.raises(ValueError):
            lat.set_spins(np.full((4, 6, 10), 3, np.int8))
        with pytest.raises(ValueError):
            lat.set_spins(np.full((4, 6, 10), -1, np.int8))
        with pytest.raises(ValueError):
            lat.sweep(0.0099, 1, 5)  # 6 |J| / T > 600
        lat.sweep(0.01, 1, 5)  # 6 |J| / T = 600 is taken
        with pytest.raises(ValueError):
            lat.cluster_sweep(1.0, 8, 5, step0=2 ** 32 - 4)
        assert (lat.get_spins() == 0).all()
    finally:
        lat.close()
    for bad in ((3, 4, 4, True), (4, 3, 4, True), (4, 4, 3, True), (1, 4, 4, True), (0, 4, 4, False), (3, 4, 4, (True, False, False))):
        with pytest.raises(ValueError):
            hip.PottsLattice3D(bad[0], bad[1], bad[2], 3, bad[3])
    for q in (1, 9):
        with pytest.raises(ValueError):
            hip.PottsLattice3D(2, 2, 2, q, False)


@pytest.mark.parametrize("depth,rows,cols,periodic,q", [(4, 5, 6, (True, False, True), 3), (18, 32, 32, ALL, 5)],
                         ids=["4x5x6-small", "18x32x32-hbm"])
@pytest.mark.parametrize("algorithm", ["heat_bath", "swendsen_wang"])
def test_run_rows_equal_the_handle_step_by_step(hip, depth, rows, cols, periodic, q, algorithm):
    """tsu_potts3d_run against single calls with a measurement after each, row for row; a run split in two equals one run; the
    launch count is that of the updates plus one measurement a row, so nothing came back to the host in between."""
    alg = hip.POTTS_HEAT_BATH if algorithm == "heat_bath" else hip.POTTS_SWENDSEN_WANG
    T, seed, c0, every, n_meas = 1.1 * T_NOMINAL, SEEDS[1], 7, 3, 6
    start = np.random.default_rng(9).integers(0, q, size=(depth, rows, cols)).astype(np.int8)
    a, b, c = (hip.PottsLattice3D(depth, rows, cols, q, periodic) for _ in range(3))
    try:
        for lat in (a, b, c):
            lat.set_spins(start)
        n0 = a.launch_count()
        a.run(T, n_meas, every, alg, seed, c0, 2)
        per_update = {"k10_3d_small": 1, "k10_3d_sweep": 2 * every, "k10_3d_sw_small": 1, "k10_3d_sw_tiles": 3 * every}[a.route(alg)]
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
            w_eq, w_N = p3.measure(b.get_spins(), q, periodic)
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
        codes.append(p3.state_code(lat.get_spins(), q))
    return codes


def _case_id(case):
    return "x".join(map(str, case[0])) + f"-q{case[1]}-" + "".join("p" if x else "o" for x in case[2]) + f"-J{case[3]:g}"


# chi^2 of the twin's chains (tests/test_potts3d_cpu.py records them with dof, p and the pooled share); the device repeats them
HEAT_BATH_CHI2 = {"2x2x2-q2-ooo-J1": "271.9", "2x2x2-q2-poo-J1": "250.4", "2x2x2-q2-ppp-J0.5": "263.7", "2x2x2-q2-ooo-J-1": "263.7",
                  "2x1x3-q3-ooo-J1": "676.3"}
CLUSTER_CHI2 = {"2x1x3-q3-ooo-J1": "667.0", "2x2x2-q2-ooo-J1": "233.9"}


@pytest.mark.parametrize("case", p3.ENUMERATION_HEAT_BATH, ids=_case_id)
def test_heat_bath_enumeration_on_the_device(hip, case):
    """The CPU test's chains on the device: the first 50 recorded states equal the twin's, and the 20 000 states give the twin's
    chi^2 to the digit (HEAT_BATH_CHI2) and pass the same check."""
    shape, q, per, J, h, T, n_states, seed = case
    lat = hip.PottsLattice3D(shape[0], shape[1], shape[2], q, per)
    try:
        lat.set_model(J, h)
        codes = _device_codes(lat, q, lambda n, c0: lat.sweep(T, n, seed, c0), 100, n_states, 4)
    finally:
        lat.close()
    s, _ = p3.chain(np.zeros(shape, np.int8), q, per, J, h, T, 100, seed)
    _, want = p3.chain(s, q, per, J, h, T, 200, seed, sweep0=100, record_every=4)
    assert codes[:50] == want
    chi2, dof, p, pooled = p3.boltzmann_chi2(codes, shape, q, per, J, h, T)
    print(f"\n{_case_id(case)}: chi2 = {chi2:.1f} on {dof} dof, p = {p:.3f}, pooled {100 * pooled:.2f} %")
    assert f"{chi2:.1f}" == HEAT_BATH_CHI2[_case_id(case)] and p >= 0.01 and pooled <= 0.05


@pytest.mark.parametrize("case", p3.ENUMERATION_CLUSTER, ids=_case_id)
def test_cluster_enumeration_on_the_device(hip, case):
    """The same for Swendsen-Wang steps (CLUSTER_CHI2)."""
    shape, q, per, J, T, n_states, seed = case
    lat = hip.PottsLattice3D(shape[0], shape[1], shape[2], q, per)
    try:
        lat.set_model(J)
        codes = _device_codes(lat, q, lambda n, c0: lat.cluster_sweep(T, n, seed, c0), 100, n_states, 4)
    finally:
        lat.close()
    s, _ = p3.cluster_chain(np.zeros(shape, np.int8), q, per, J, T, 100, seed)
    _, want = p3.cluster_chain(s, q, per, J, T, 200, seed, step0=100, record_every=4)
    assert codes[:50] == want
    chi2, dof, p, pooled = p3.boltzmann_chi2(codes, shape, q, per, J, None, T)
    print(f"\n{_case_id(case)}: chi2 = {chi2:.1f} on {dof} dof, p = {p:.3f}, pooled {100 * pooled:.2f} %")
    assert f"{chi2:.1f}" == CLUSTER_CHI2[_case_id(case)] and p >= 0.01 and pooled <= 0.05


def _batch_means(x, n_batches=20):
    x = np.asarray(x, dtype=np.float64)
    b = x[: len(x) // n_batches * n_batches].reshape(n_batches, -1).mean(axis=1)
    return float(x.mean()), float(b.std(ddof=1) / math.sqrt(n_batches))


T_Q3 = 1.8163  # the weak first-order transition of q = 3 on the cubic lattice, in units of J


@pytest.mark.parametrize("factor", [0.85, 1.15])
def test_heat_bath_and_cluster_steps_agree_at_q3(factor):
    """8 x 8 x 8 periodic, q = 3, T = factor x 1.8163 (away from the first-order point): <e> and <m> of the two algorithms within 4
    combined batch-means errors.  Run lengths from the twin at this shape (4000 sweeps / 2500 steps after 300, windowed sum of the
    autocorrelation function): tau_int of (e, m) is (1.24, 1.32) sweeps and (3.50, 3.76) steps at 0.85, (1.22, 2.41) sweeps and
    (1.17, 0.74) steps at 1.15.  Here: 500 updates discarded, then 4000 measurements 4 updates apart in 20 batches: a batch is 800
    updates, 330 times the longest tau_int of the sweeps and 210 times that of the steps."""
    import tsu
    T = factor * T_Q3
    res = {}
    for algorithm in ("heat_bath", "swendsen_wang"):
        model = tsu.PottsModel3D(8, 3, temperature=T, seed=21)
        model.equilibrate(n_sweeps=500, algorithm=algorithm)
        rows = model.run(4000, 4, algorithm)
        model.close()
        res[algorithm] = (_batch_means(-rows[:, 0] / 512.0), _batch_means(p3.order_parameter(rows[:, 1:], 3)))
    for k, name in enumerate(("e", "m")):
        (a, ea), (b, eb) = res["heat_bath"][k], res["swendsen_wang"][k]
        print(f"\n{factor} x 1.8163 <{name}>: heat bath {a:.5f} +- {ea:.5f}, cluster {b:.5f} +- {eb:.5f}")
        assert abs(a - b) <= 4.0 * math.hypot(ea, eb)


@pytest.mark.parametrize("T", [4.0, 5.0])
def test_q2_agrees_with_the_ising_model(T):
    """q = 2 is the Ising model under J_Potts = 2 J_Ising: at 6 x 6 x 6 periodic with coupling 2.0, <n_eq> agrees with
    (N_b - E_Ising / J) / 2 of IsingModel3D within 4 combined batch-means errors.  tau_int of n_eq from the twin at this shape (4000
    sweeps after 300): 3.0 sweeps at T = 4.0, 2.5 at T = 5.0; the Ising sweep is the same conditional law.  Here, each side: 500
    sweeps discarded, 2000 measurements 5 sweeps apart, 20 batches of 500 sweeps, 165 tau_int."""
    import tsu
    n_b = 3 * 216
    potts = tsu.PottsModel3D(6, 2, temperature=T, coupling=2.0, seed=31)
    potts.equilibrate(n_sweeps=500)
    rows = potts.run(2000, 5)
    potts.close()
    ising = tsu.IsingModel3D(size=6, coupling=1.0, temperature=T, seed=32)
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
    per = (True, False, True)
    m = tsu.PottsModel3D((4, 5, 6), 3, temperature=1.0, field=(0.1, 0.0, -0.1), periodic=per, seed=5)
    start = np.random.default_rng(5).integers(0, 3, size=(4, 5, 6)).astype(np.int8)
    assert (m.spins == start).all() and m.route() == "k10_3d_small" and m.route("swendsen_wang") == "k10_3d_sw_small"
    m.gibbs_update(2).gibbs_update(1)
    want = p3.sweep(start, 3, per, 1.0, (0.1, 0.0, -0.1), 1.0, 3, 5)
    assert (m.spins == want).all() and m.sweep_count == 3
    assert m.energy() == p3.energy(want, 3, per, 1.0, (0.1, 0.0, -0.1))
    assert m.equal_bonds() == p3.measure(want, 3, per)[0]
    assert m.colour_counts().tolist() == p3.measure(want, 3, per)[1].tolist()
    assert m.order_parameter() == p3.order_parameter(p3.measure(want, 3, per)[1], 3)
    with pytest.raises(tsu._hip.UnsupportedError):
        m.cluster_update()
    with pytest.raises(ValueError):
        m.spins = np.full((4, 5, 6), 3)
    with pytest.raises(ValueError):
        m.spins = np.ones((5, 6), np.int64)
    m.spins = np.ones((4, 5, 6), np.int64)
    assert (m.fill(2).spins == 2).all() and m.launch_count() >= 2
    m.close()
    c = tsu.PottsModel3D((4, 5, 6), 3, temperature=1.7, periodic=per, seed=6, initial=1)
    assert (c.spins == 1).all()
    c.cluster_update(2).cluster_update(1)
    assert (c.spins == p3.cluster_sweep(np.ones((4, 5, 6), np.int8), 3, per, 1.0, 1.7, 3, 6)).all() and c.cluster_count == 3
    rows = c.run(3, 2, "swendsen_wang")
    assert rows.shape == (3, 4) and c.cluster_count == 9 and rows[-1, 0] == c.equal_bonds()
    c.close()
    res = tsu.potts_temperature_scan_3d(4, 3, [0.5, 6.0], n_equilibrate=200, n_measure=100, measure_every=2, algorithm="swendsen_wang", seed=3)
    assert res["order_parameter"][0] > 0.9 > 0.5 > res["order_parameter"][1] and res["energy"][0] < res["energy"][1]
    assert sorted(res) == sorted(["energy", "order_parameter", "specific_heat", "susceptibility", "binder", "temperatures"])
    assert all(res[k].shape == (2,) for k in ("specific_heat", "susceptibility", "binder"))

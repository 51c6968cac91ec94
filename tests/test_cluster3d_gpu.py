"""K8 Swendsen-Wang cluster steps of 3-D lattices on the GPU (csrc/ising3d_cluster.hip): bit-exact against the NumPy twin
(tests/helpers/cluster3d_twin.py) on both routes, five kinds of couplings and any tile shape; the launch counts of the routes and
the batch; one layer against K6 on the device; a cluster across every seam and wrap; interleaving with heat-bath sweeps; the
errors; exact enumeration of two small open lattices; 16^3 against the heat-bath kernel; the decorrelation at T_c on 32^3; the
Python API."""
import importlib.util
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


twin = _load("cluster3d_twin")
twin2 = _load("cluster_twin")
lat3 = _load("lattice3d_twin")

TC3 = 4.5115
KINDS = ["ferro", "antiferro", "gauss", "pmJ", "diluted"]


@pytest.fixture(scope="module")
def hip():
    from tsu import _hip
    return _hip


@pytest.fixture(autouse=True)
def _no_tile_switch(monkeypatch):
    monkeypatch.delenv("TSU_SW3D_TILE", raising=False)


def _disorder(kind, shape, periodic, dseed):
    """(J_right, J_down, J_layer) float32; the last slice of an open axis 0."""
    rng = np.random.default_rng(dseed)
    if kind == "ferro":
        j = [np.full(shape, 1.0, np.float32) for _ in range(3)]
    elif kind == "antiferro":
        j = [np.full(shape, -1.0, np.float32) for _ in range(3)]
    elif kind == "gauss":
        j = [rng.normal(size=shape).astype(np.float32) for _ in range(3)]
    elif kind == "pmJ":
        j = [rng.choice(np.array([-1.0, 1.0], np.float32), size=shape) for _ in range(3)]
    elif kind == "diluted":
        j = [np.where(rng.random(shape) < 0.3, 0.0, 1.0).astype(np.float32) for _ in range(3)]
    else:
        raise ValueError(kind)
    pz, pr, pc = twin.axes(periodic)
    if not pc:
        j[0][:, :, -1] = 0.0
    if not pr:
        j[1][:, -1, :] = 0.0
    if not pz:
        j[2][-1, :, :] = 0.0
    return tuple(j)


def _same(got, want, what):
    assert (got == want).all(), f"{what}: differs at {np.argwhere(got != want)[:5].tolist()} ({int((got != want).sum())} sites)"


def _check_calls(hip, shape, periodic, kind, T, calls, seed=77, replica=0, dseed=5, start="random"):
    """Random start, then `calls` = [(step0, n_steps), ...]; every call compared with the twin bit for bit."""
    j = _disorder(kind, shape, periodic, dseed)
    lat = hip.Lattice3D(*shape, periodic)
    try:
        if start == "random":
            lat.randomize(seed + 1)
        else:
            lat.fill(1)
        lat.set_disorder(*j)
        want = lat.get_spins()
        for step0, n in calls:
            lat.cluster_sweep(T, n, seed, step0, replica)
            want = twin.sweep(want, periodic, *j, T, n, seed, step0, replica)
            _same(lat.get_spins(), want, f"{shape} periodic={periodic} {kind} T={T} step0={step0}")
        return want, lat.cluster_launch_count()
    finally:
        lat.close()


SMALL_SHAPES = [((1, 5, 7), False), ((3, 4, 6), False), ((5, 7, 9), False), ((4, 6, 8), True), ((2, 3, 300), False),
                ((8, 16, 32), (True, False, True)), ((7, 8, 6), (False, True, True)), ((6, 9, 4), (True, False, False)),
                ((16, 32, 32), True)]


@pytest.mark.parametrize("shape,periodic", SMALL_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_bit_exact_small_route(hip, shape, periodic, kind):
    T = {"ferro": 4.5, "antiferro": 3.0, "gauss": 1.2, "pmJ": 2.0, "diluted": 2.5}[kind]
    _, launches = _check_calls(hip, shape, periodic, kind, T, [(0, 1), (1, 3), (40, 2)])
    assert launches == 3  # one launch per call


TILED_SHAPES = [((20, 40, 70), False), ((32, 32, 32), True), ((20, 36, 34), (True, False, False)),
                ((20, 36, 34), (False, True, False)), ((20, 36, 34), (False, False, True)), ((9, 50, 66), (False, True, True))]


@pytest.mark.parametrize("shape,periodic", TILED_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_bit_exact_tiled_route(hip, shape, periodic, kind):
    """More than 16384 sites: 8 x 16 x 32 tiles, shapes that do not divide into them, several tiles on every axis (20 x 40 x 70:
    3 x 3 x 3), each axis periodic in turn."""
    T = {"ferro": 4.5115, "antiferro": 3.0, "gauss": 1.2, "pmJ": 2.0, "diluted": 2.5}[kind]
    _, launches = _check_calls(hip, shape, periodic, kind, T, [(0, 1), (1, 2)])
    assert launches == 9  # three launches per step


def test_large_default_tile(hip, monkeypatch):
    """16 x 32 x 32 tiles (the default once they fill the chip), forced here on a lattice of 3 x 3 x 2 of them with ragged edges."""
    monkeypatch.setenv("TSU_SW3D_TILE", "16x32x32")
    _check_calls(hip, (36, 70, 64), (False, False, True), "ferro", 4.5115, [(3, 2)])
    _check_calls(hip, (36, 70, 64), (False, False, True), "gauss", 1.0, [(3, 1)])


def test_split_calls_and_replicas(hip):
    for shape, periodic in (((4, 6, 8), True), ((20, 36, 34), (True, False, False))):
        one, _ = _check_calls(hip, shape, periodic, "gauss", 1.5, [(5, 6)])
        many, _ = _check_calls(hip, shape, periodic, "gauss", 1.5, [(5, 1), (6, 2), (8, 3)])
        _same(one, many, f"{shape}: one call of 6 steps against 3 calls")
        other, _ = _check_calls(hip, shape, periodic, "gauss", 1.5, [(5, 6)], replica=2)
        assert (other != one).any()


TILES = ["1x1x2", "2x2x2", "4x4x4", "3x5x6", "8x16x32", "16x32x32", "2x64x8"]


@pytest.mark.parametrize("shape,periodic,kind", [((6, 10, 12), (True, False, True), "ferro"), ((5, 7, 9), False, "gauss"),
                                                 ((1, 5, 7), False, "pmJ"), ((8, 12, 20), True, "diluted")])
def test_same_spins_for_every_tile_shape(hip, monkeypatch, shape, periodic, kind):
    small, n = _check_calls(hip, shape, periodic, kind, 2.5, [(2, 3), (40, 2)])
    assert n == 2
    for tile in TILES:
        monkeypatch.setenv("TSU_SW3D_TILE", tile)
        out, n = _check_calls(hip, shape, periodic, kind, 2.5, [(2, 3), (40, 2)])
        _same(out, small, f"{shape} tile {tile}")
        assert n > 2  # the tiled route


def test_routes_by_launch_count(hip):
    shape = (8, 16, 16)
    j = _disorder("gauss", shape, True, 3)
    small = hip.Lattice3D(*shape, True)
    small.randomize(1)
    small.set_disorder(*j)
    small.cluster_sweep(2.0, 1, 5, 0)
    assert small.cluster_launch_count() == 1
    small.cluster_sweep(2.0, 25, 5, 1)
    assert small.cluster_launch_count() == 2          # one launch per call, whatever n_steps is
    assert small.launch_count() == 0                  # the sweep-kernel count is not touched
    small.cluster_sweep(2.0, 0, 5, 26)
    assert small.cluster_launch_count() == 2          # n_steps = 0 launches nothing
    small.close()
    # a batch of 8 small lattices of one shape, each with its own disorder: ONE launch, same spins as the twin (and as serial calls)
    shape, per = (5, 12, 10), (False, True, True)
    lats = [hip.Lattice3D(*shape, per) for _ in range(8)]
    serial = [hip.Lattice3D(*shape, per) for _ in range(8)]
    dis = [_disorder(KINDS[i % 5], shape, per, 20 + i) for i in range(8)]
    Ts = np.linspace(1.5, 5.0, 8)
    for i in range(8):
        for l in (lats[i], serial[i]):
            l.randomize(100 + i)
            l.set_disorder(*dis[i])
    starts = [l.get_spins() for l in lats]
    hip.cluster_sweep_batch_3d(lats, 4, Ts, [7 + i for i in range(8)], [3 * i for i in range(8)], list(range(8)))
    for i in range(8):
        serial[i].cluster_sweep(Ts[i], 4, 7 + i, 3 * i, i)
        assert lats[i].cluster_launch_count() == 1 and lats[i].launch_count() == 0
        got = lats[i].get_spins()
        _same(got, twin.sweep(starts[i], per, *dis[i], Ts[i], 4, 7 + i, 3 * i, i), f"batch lattice {i}")
        _same(got, serial[i].get_spins(), f"batch lattice {i} against the serial call")
    # lattices of two shapes: one call per lattice, the same spins
    odd = hip.Lattice3D(3, 4, 6, False)
    odd.fill(1)
    jo = _disorder("ferro", (3, 4, 6), False, 0)
    odd.set_disorder(*jo)
    hip.cluster_sweep_batch_3d([lats[0], odd], 2, [2.0, 3.0], [1, 2], [0, 0])
    _same(odd.get_spins(), twin.sweep(np.ones((3, 4, 6), np.int8), False, *jo, 3.0, 2, 2, 0), "mixed batch")
    assert lats[0].cluster_launch_count() == 2 and odd.cluster_launch_count() == 1
    for l in lats + serial + [odd]:
        l.close()
    # a large lattice: three launches per step
    big = hip.Lattice3D(32, 32, 32, True)
    big.randomize(2)
    big.set_disorder(*_disorder("ferro", (32, 32, 32), True, 0))
    big.cluster_sweep(TC3, 1, 5, 0)
    per_step = big.cluster_launch_count()
    big.cluster_sweep(TC3, 7, 5, 1)
    assert per_step == 3 and big.cluster_launch_count() == 8 * per_step and big.launch_count() == 0
    big.close()


@pytest.mark.parametrize("rows,cols,periodic,J,T", [(24, 40, True, 1.0, 2.269), (13, 21, False, 1.0, 3.0), (16, 12, True, -1.0, 2.0),
                                                    (160, 200, True, 1.0, 2.269)])
def test_one_layer_equals_k6_on_the_device(hip, rows, cols, periodic, J, T):
    l2 = hip.Lattice(rows, cols, periodic)
    l3 = hip.Lattice3D(1, rows, cols, (False, periodic, periodic))
    try:
        for lat in (l2, l3):
            lat.randomize(9)
        jr, jd, jl = (np.full((1, rows, cols), J, np.float32) for _ in range(3))
        jl[:] = 0.0
        if not periodic:
            jr[:, :, -1] = 0.0
            jd[:, -1, :] = 0.0
        l3.set_disorder(jr, jd, jl)
        for step0, n in ((0, 3), (3, 2)):
            l2.cluster_sweep(J, T, n, 31, step0, 1)
            l3.cluster_sweep(T, n, 31, step0, 1)
            _same(l3.get_spins()[0], l2.get_spins(), f"one layer {rows}x{cols} step0={step0}")
    finally:
        l2.close()
        l3.close()


@pytest.mark.parametrize("J", [1.0, -1.0])
@pytest.mark.parametrize("rows,cols,periodic", [(37, 53, False), (24, 40, True)])
def test_one_layer_equals_k6_on_the_tiled_route(hip, monkeypatch, rows, cols, periodic, J):
    """The shapes above stay on the one-workgroup route.  Here both handles are forced onto tiles of 8 x 8 sites (ragged last tiles
    at 37 x 53, the two wraps at 24 x 40): local, merge and resolve of K6 against the same three kernels of K8 on one layer."""
    monkeypatch.setenv("TSU_SW_TILE", "8")
    monkeypatch.setenv("TSU_SW3D_TILE", "1x8x8")
    T = 2.269
    l2 = hip.Lattice(rows, cols, periodic)
    l3 = hip.Lattice3D(1, rows, cols, (False, periodic, periodic))
    try:
        for lat in (l2, l3):
            lat.randomize(9)
        _same(l3.get_spins()[0], l2.get_spins(), f"one layer {rows}x{cols}: the start")
        jr, jd, jl = _disorder("ferro" if J > 0 else "antiferro", (1, rows, cols), (False, periodic, periodic), 0)
        l3.set_disorder(jr, jd, jl)
        l2.cluster_sweep(J, T, 3, 31, 5, 1)
        l3.cluster_sweep(T, 3, 31, 5, 1)
        _same(l3.get_spins()[0], l2.get_spins(), f"one layer {rows}x{cols} J={J} on tiles")
        assert l2.cluster_launch_count() == 9 and l3.cluster_launch_count() == 9
    finally:
        l2.close()
        l3.close()


@pytest.mark.parametrize("shape", [(24, 36, 68), (8, 16, 32)])
def test_one_cluster_across_every_seam_and_wrap(hip, shape):
    """All up, periodic, T = 0.01: every bond is active, one cluster spans all seams and the three wraps; the result is uniform."""
    want, _ = _check_calls(hip, shape, True, "ferro", 0.01, [(0, 1), (1, 3)], seed=13, start="up")
    assert abs(int(want.sum())) == want.size
    roots, act = twin.labels(want, True, *_disorder("ferro", shape, True, 0), 0.01, 13, 4)
    assert (roots == 0).all() and all(a.all() for a in act)


def test_interleaving_with_heat_bath_sweeps(hip):
    from tsu.models.ising import IsingModel3D
    shape, per, T, seed = (6, 8, 12), (True, False, True), 2.2, 4242
    j = _disorder("gauss", shape, per, 8)
    m = IsingModel3D(shape, temperature=T, periodic=per, seed=seed, initial="up", couplings=j)
    s = np.ones(shape, np.int8)
    m.gibbs_update(3)
    s = lat3.sweep(s, per, *j, None, T, 3, seed, 0)
    m.cluster_update(4)
    s = twin.sweep(s, per, *j, T, 4, seed, 0)
    m.gibbs_update(2)
    s = lat3.sweep(s, per, *j, None, T, 2, seed, 3)
    assert m.sweep_count == 5 and m.cluster_count == 4
    _same(m.spins, s, "interleaved")
    m.equilibrate(n_sweeps=2, algorithm="swendsen_wang")
    _same(m.spins, twin.sweep(s, per, *j, T, 2, seed, 4), "equilibrate(swendsen_wang)")
    assert m.cluster_count == 6 and m.sweep_count == 5
    assert m._lat.launch_count() == 10 and m._lat.cluster_launch_count() == 2
    m.equilibrate(n_sweeps=1)
    assert m.sweep_count == 6 and m.cluster_count == 6 and m._lat.launch_count() == 12


def test_errors(hip, monkeypatch):
    shape = (4, 6, 8)
    j = _disorder("ferro", shape, False, 0)
    lat = hip.Lattice3D(*shape, False)
    try:
        lat.fill(1)
        with pytest.raises(ValueError, match="set_disorder first"):
            lat.cluster_sweep(2.0, 1, 1, 0)
        h = np.zeros(shape, np.float32)
        h[2, 3, 4] = -0.5
        lat.set_disorder(*j, h)
        with pytest.raises(hip.UnsupportedError, match="ghost spin"):
            lat.cluster_sweep(2.0, 1, 1, 0)
        with pytest.raises(hip.UnsupportedError, match="ghost spin"):
            hip.cluster_sweep_batch_3d([lat], 1, [2.0], [1], [0])
        lat.set_disorder(*j, np.zeros(shape, np.float32))  # an all-zero h is zero field
        for T in (0.0, -1.0):
            with pytest.raises(ValueError, match="Temperature must be positive"):
                lat.cluster_sweep(T, 1, 1, 0)
            with pytest.raises(ValueError, match="Temperature must be positive"):
                hip.cluster_sweep_batch_3d([lat], 1, [T], [1], [0])
        with pytest.raises(ValueError):
            lat.cluster_sweep(2.0, -1, 1, 0)
        with pytest.raises(ValueError, match="twice"):
            hip.cluster_sweep_batch_3d([lat, lat], 1, [2.0, 2.0], [1, 2], [0, 0])
        monkeypatch.setenv("TSU_SW3D_TILE", "4x4x3")
        with pytest.raises(ValueError, match="even width"):
            lat.cluster_sweep(2.0, 1, 1, 0)
        monkeypatch.setenv("TSU_SW3D_TILE", "4x4")
        with pytest.raises(ValueError, match="TSU_SW3D_TILE"):
            lat.cluster_sweep(2.0, 1, 1, 0)
        monkeypatch.delenv("TSU_SW3D_TILE")
        assert (lat.get_spins() == 1).all()
        lat.cluster_sweep(2.0, 0, 1, 0)
        assert lat.cluster_launch_count() == 0 and lat.launch_count() == 0
        lat.set_disorder(*j)  # a NULL h is zero field
        lat.cluster_sweep(2.0, 2, 1, 0)
        assert lat.cluster_launch_count() == 1 and lat.launch_count() == 0
    finally:
        lat.close()


ENUM_SAMPLES = {(2, 2, 2): 20000, (2, 3, 2): 100000}


@pytest.mark.parametrize("shape,T,seed,dseed", [((2, 2, 2), 2.0, 11, 3), ((2, 3, 2), 1.5, 13, 5)])
def test_exact_enumeration(hip, shape, T, seed, dseed):
    """The step samples exp(-E / T) / Z at zero field: open lattices from all up, the couplings of
    lattice3d_twin.enumeration_disorder with the field replaced by zeros; 100 steps discarded, then 20 000 (2 x 2 x 2) or 100 000
    (2 x 3 x 2) states taken every 4 steps with the step counter running on; chi^2 of the state histogram over the states with
    expected count >= 5, the rest pooled.  The NumPy twin (bit-identical to the device) gives at these seeds
    chi^2 = 132.8 on 150 d.o.f. (p = 0.84, pooled 0.80 %) and 1264.2 on 1226 d.o.f. (p = 0.22, pooled 2.81 %)."""
    jr, jd, jl, _ = lat3.enumeration_disorder(shape, dseed)
    d = (jr, jd, jl, np.zeros(shape, np.float32))
    lat = hip.Lattice3D(*shape, False)
    try:
        lat.fill(1)
        lat.set_disorder(jr, jd, jl)
        lat.cluster_sweep(T, 100, seed, 0)
        want = twin.sweep(np.ones(shape, np.int8), False, jr, jd, jl, T, 100, seed, 0)
        _same(lat.get_spins(), want, f"enumeration {shape}: burn-in")
        codes, steps = [], 100
        for k in range(ENUM_SAMPLES[shape]):
            lat.cluster_sweep(T, 4, seed, steps)
            steps += 4
            s = lat.get_spins()
            if k < 50:
                want = twin.sweep(want, False, jr, jd, jl, T, 4, seed, steps - 4)
                _same(s, want, f"enumeration {shape}: state {k}")
            codes.append(lat3.state_code(s))
    finally:
        lat.close()
    chi2, dof, p, pooled = lat3.boltzmann_chi2(codes, shape, d, T)
    print(f"\n{shape} T = {T}: chi2 = {chi2:.1f} on {dof} d.o.f., p = {p:.3f}, pooled share {pooled:.2%}")
    assert p >= 0.01, (chi2, dof, p)
    assert pooled <= 0.05, pooled


@pytest.mark.parametrize("T", [4.0, 5.0])
def test_equilibrium_at_16_cubed_against_heat_bath(hip, T):
    """Periodic 16^3, J = 1: <E> / N and <|m|> from Swendsen-Wang and from k8_sweep, 20 batch means each, within 4 combined
    batch-means errors (the rule of K6's 512^2 test)."""
    from tsu.models.ising import IsingModel3D
    n_batches, per = 20, 100

    def series(advance, burn):
        m = IsingModel3D(16, temperature=T, seed=31, initial="up")
        advance(m, burn)
        E, M = np.zeros((n_batches, per)), np.zeros((n_batches, per))
        for b in range(n_batches):
            for k in range(per):
                advance(m, 1)
                E[b, k] = m.energy() / m.n_spins
                M[b, k] = abs(m.magnetization())
        e_b, m_b = E.mean(axis=1), M.mean(axis=1)
        return (e_b.mean(), e_b.std(ddof=1) / math.sqrt(n_batches), m_b.mean(), m_b.std(ddof=1) / math.sqrt(n_batches))

    e_sw, de_sw, m_sw, dm_sw = series(lambda m, n: m.cluster_update(n), 200)
    e_hb, de_hb, m_hb, dm_hb = series(lambda m, n: m.gibbs_update(10 * n), 100)
    print(f"\n16^3 T = {T}: E/N SW {e_sw:.5f} +- {de_sw:.5f}, heat-bath {e_hb:.5f} +- {de_hb:.5f}; "
          f"|m| SW {m_sw:.5f} +- {dm_sw:.5f}, heat-bath {m_hb:.5f} +- {dm_hb:.5f}")
    assert abs(e_sw - e_hb) < 4 * math.hypot(de_sw, de_hb), (e_sw, e_hb, de_sw, de_hb)
    assert abs(m_sw - m_hb) < 4 * math.hypot(dm_sw, dm_hb), (m_sw, m_hb, dm_sw, dm_hb)


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
    """Periodic 32^3 at T_c = 4.5115: tau_int(|m|) of heat-bath sweeps is at least 5 times that of Swendsen-Wang steps (a floor
    that guards against a step that does not decorrelate; the measured values are in DESIGN.md section 5)."""
    from tsu.models.ising import IsingModel3D
    m = IsingModel3D(32, temperature=TC3, seed=17)
    m.cluster_update(1000)
    n = 20000
    sw = np.empty(n)
    for i in range(n):
        m.cluster_update(1)
        sw[i] = abs(m.magnetization())
    every = 8
    hb = np.empty(n)
    for i in range(n):
        m.gibbs_update(every)
        hb[i] = abs(m.magnetization())
    tau_sw, tau_hb = _tau_int(sw), every * _tau_int(hb)
    print(f"\n32^3 at T_c: tau_int(|m|) SW {tau_sw:.2f} steps, heat-bath {tau_hb:.1f} sweeps, ratio {tau_hb / tau_sw:.1f}")
    assert tau_hb >= 5 * tau_sw, (tau_sw, tau_hb)


def test_temperature_scan_batch_equals_serial(hip):
    from tsu.models.ising import IsingModel3D, temperature_scan_3d
    temps = [3.5, 4.0, 4.5115, 5.5]
    shape = (6, 8, 12)
    out = temperature_scan_3d(shape, temps, n_equilibrate=10, n_measure=6, measure_every=3, seed=5, algorithm="swendsen_wang",
                              replicas=2)
    for i, T in enumerate(temps):
        m = IsingModel3D(shape, temperature=T, seed=5 + i, initial="up")
        m2 = IsingModel3D(shape, temperature=T, seed=5 + len(temps) + i, initial="up")
        m.cluster_update(10)
        m2.cluster_update(10)
        Ms, Es, Qs = [], [], []
        for _ in range(6):
            m.cluster_update(3)
            m2.cluster_update(3)
            Ms.append(m.magnetization())
            Es.append(m.energy())
            Qs.append(m.overlap(m2))
        Ms, Es, Qs = np.array(Ms), np.array(Es), np.array(Qs)
        assert out["magnetization"][i] == np.mean(np.abs(Ms))
        assert out["energy"][i] == np.mean(Es) / m.n_spins
        assert out["susceptibility"][i] == (np.mean(Ms ** 2) - np.mean(np.abs(Ms)) ** 2) * m.n_spins / T
        assert out["specific_heat"][i] == (np.mean(Es ** 2) - np.mean(Es) ** 2) / (T ** 2 * m.n_spins)
        assert out["overlap"][i] == np.mean(np.abs(Qs))
        assert m.sweep_count == 0 and m.cluster_count == 28
    # the default algorithm is the heat-bath scan it was
    a = temperature_scan_3d(shape, temps[:2], n_equilibrate=4, n_measure=3, measure_every=2, seed=5)
    b = temperature_scan_3d(shape, temps[:2], n_equilibrate=4, n_measure=3, measure_every=2, seed=5, algorithm="gibbs")
    for i, T in enumerate(temps[:2]):
        m = IsingModel3D(shape, temperature=T, seed=5 + i, initial="up")
        m.gibbs_update(4)
        Ms = []
        for _ in range(3):
            m.gibbs_update(2)
            Ms.append(m.magnetization())
        assert a["magnetization"][i] == b["magnetization"][i] == np.mean(np.abs(Ms))
        assert m._lat.cluster_launch_count() == 0

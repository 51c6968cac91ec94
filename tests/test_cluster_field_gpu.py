"""K8 ghost-spin Swendsen-Wang steps on the GPU (csrc/ising3d_cluster.hip, tsu_ising3d_cluster_sweep_field): bit-exact against the
NumPy twin (tests/helpers/cluster_field_twin.py) on both routes; zero field against the zero-field entry point; freezing across
every seam and wrap; two slabs; the batch; exact enumeration of two small open lattices in a Gaussian field; 16^3 in a field against
the heat-bath kernel; the Python API."""
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


twin = _load("cluster_field_twin")
twin0 = _load("cluster3d_twin")
lat3 = _load("lattice3d_twin")

TC3 = 4.5115


@pytest.fixture(scope="module")
def hip():
    from tsu import _hip
    return _hip


@pytest.fixture(autouse=True)
def _no_tile_switch(monkeypatch):
    monkeypatch.delenv("TSU_SW3D_TILE", raising=False)


def _open_edges(j, periodic):
    pz, pr, pc = twin.axes(periodic)
    if not pc:
        j[0][:, :, -1] = 0.0
    if not pr:
        j[1][:, -1, :] = 0.0
    if not pz:
        j[2][-1, :, :] = 0.0
    return tuple(j)


def _disorder(kind, shape, periodic, dseed):
    """(J_right, J_down, J_layer, h) float32 and a temperature for them."""
    rng = np.random.default_rng(dseed)
    if kind == "gauss":  # Gaussian J + Gaussian h
        j = [rng.normal(size=shape).astype(np.float32) for _ in range(3)]
        h, T = rng.normal(size=shape).astype(np.float32), 1.2
    elif kind == "pmJ":  # +-J + bimodal h
        j = [rng.choice(np.array([-1.0, 1.0], np.float32), size=shape) for _ in range(3)]
        h, T = rng.choice(np.array([-0.7, 0.7], np.float32), size=shape), 2.0
    elif kind in ("ferro+", "ferro-"):  # ferromagnet + uniform h of either sign
        j = [np.full(shape, 1.0, np.float32) for _ in range(3)]
        h, T = np.full(shape, 0.3 if kind == "ferro+" else -0.3, np.float32), 4.0
    else:
        raise ValueError(kind)
    return _open_edges(j, periodic) + (h,), T


FIELD_KINDS = ["gauss", "pmJ", "ferro+", "ferro-"]


def _same(got, want, what):
    assert (got == want).all(), f"{what}: differs at {np.argwhere(got != want)[:5].tolist()} ({int((got != want).sum())} sites)"


def _check_calls(hip, shape, periodic, d, T, calls, seed=77, replica=0, start="random"):
    """Random start, then `calls` = [(step0, n_steps), ...]; every call compared with the twin bit for bit."""
    lat = hip.Lattice3D(*shape, periodic)
    try:
        if start == "random":
            lat.randomize(seed + 1)
        else:
            lat.fill(1)
        lat.set_disorder(*d)
        want = lat.get_spins()
        for step0, n in calls:
            lat.cluster_sweep_field(T, n, seed, step0, replica)
            want = twin.sweep(want, periodic, *d, T, n, seed, step0, replica)
            _same(lat.get_spins(), want, f"{shape} periodic={periodic} T={T} step0={step0} replica={replica}")
        return want, lat.cluster_launch_count()
    finally:
        lat.close()


CALLS = [(0, 1), (1, 3), (40, 2)]


@pytest.mark.parametrize("kind", FIELD_KINDS)
@pytest.mark.parametrize("shape,periodic", [((4, 6, 8), False), ((4, 4, 8), True), ((3, 5, 7), False),
                                            ((1, 6, 10), (False, True, True))])
def test_bit_exact_small_route(hip, shape, periodic, kind):
    d, T = _disorder(kind, shape, periodic, 5)
    for replica in (0, 3):
        _, launches = _check_calls(hip, shape, periodic, d, T, CALLS, replica=replica)
        assert launches == 3  # one launch per call


@pytest.mark.parametrize("kind", FIELD_KINDS)
@pytest.mark.parametrize("shape,periodic,tile", [((4, 6, 8), False, "2x3x4"), ((8, 8, 16), True, "4x4x8"), ((8, 8, 16), True, "3x5x6")])
def test_bit_exact_tiled_route(hip, monkeypatch, shape, periodic, tile, kind):
    monkeypatch.setenv("TSU_SW3D_TILE", tile)
    d, T = _disorder(kind, shape, periodic, 6)
    for replica in (0, 3):
        _, launches = _check_calls(hip, shape, periodic, d, T, CALLS, replica=replica)
        assert launches == 18  # three launches per step: every one of these lattices has seams


def test_a_field_changes_the_spins(hip):
    """The parity tests are not vacuous: with these fields the steps differ from the zero-field ones."""
    shape, periodic = (4, 4, 8), True
    for kind in FIELD_KINDS:
        d, T = _disorder(kind, shape, periodic, 5)
        got, _ = _check_calls(hip, shape, periodic, d, T, [(0, 4)])
        start = hip.Lattice3D(*shape, periodic)
        start.randomize(78)
        zero = twin0.sweep(start.get_spins(), periodic, *d[:3], T, 4, 77, 0)
        start.close()
        assert (got != zero).any(), kind


@pytest.mark.parametrize("tile", [None, "2x3x4", "3x5x6"])
def test_zero_field_equals_the_zero_field_entry_point(hip, monkeypatch, tile):
    """h NULL and h all zeros, both routes: the spins and the launch counts of tsu_ising3d_cluster_sweep."""
    if tile:
        monkeypatch.setenv("TSU_SW3D_TILE", tile)
    shape, periodic = (4, 6, 8), (True, False, True)
    d, T = _disorder("gauss", shape, periodic, 8)
    for h in (None, np.zeros(shape, np.float32)):
        old, new = hip.Lattice3D(*shape, periodic), hip.Lattice3D(*shape, periodic)
        try:
            for lat in (old, new):
                lat.randomize(3)
                lat.set_disorder(*d[:3], h)
            for step0, n in CALLS:
                old.cluster_sweep(T, n, 9, step0, 2)
                new.cluster_sweep_field(T, n, 9, step0, 2)
                _same(new.get_spins(), old.get_spins(), f"zero field, tile {tile}, step0={step0}")
            assert new.cluster_launch_count() == old.cluster_launch_count() == (18 if tile else 3)
            assert new.launch_count() == 0
        finally:
            old.close()
            new.close()


@pytest.mark.parametrize("tile", ["4x4x8", None])
def test_freezing_crosses_every_seam_and_wrap(hip, monkeypatch, tile):
    """J = 1, T = 1e-3, all up, periodic 8 x 8 x 16: every bond is active (thr = 2^32), the lattice is one cluster.  One site in the
    last tile carries a field.  h = +5 there: its ghost bond is active at every step, the whole lattice is frozen.  h = -5: the
    bond is unsatisfied while the spins are up, so the lattice flips as one cluster by the coin of site 0 until it is all down;
    from then on the bond is satisfied and active and nothing changes."""
    if tile:
        monkeypatch.setenv("TSU_SW3D_TILE", tile)
    shape, T, seed = (8, 8, 16), 1e-3, 13
    j = tuple(np.ones(shape, np.float32) for _ in range(3))
    assert twin.thresholds(np.float32(1.0), T) == 2 ** 32 and twin.thresholds(np.float32(5.0), T) == 2 ** 32
    for sign in (1.0, -1.0):
        h = np.zeros(shape, np.float32)
        h[7, 6, 13] = 5.0 * sign
        lat = hip.Lattice3D(*shape, True)
        try:
            lat.fill(1)
            lat.set_disorder(*j, h)
            down = False
            for t in range(8):
                lat.cluster_sweep_field(T, 1, seed, t)
                s = lat.get_spins()
                if sign < 0 and not down:
                    down = bool(twin.flip_of_roots(np.array([0]), shape[2], seed, t)[0])
                want = -1 if down else 1
                assert (s == want).all(), f"h = {5 * sign:+}, tile {tile}, step {t}: {int((s != want).sum())} sites differ"
            assert down == (sign < 0)  # at this seed site 0's coin comes up within 8 steps
            assert lat.cluster_launch_count() == (24 if tile else 8)
        finally:
            lat.close()


@pytest.mark.parametrize("tile", [None, "2x4x8"])
def test_two_slabs(hip, monkeypatch, tile):
    """A zero J_layer plane (and the open z axis) separates layers 0-1 from layers 2-3.  Cold and all up, each slab is one cluster:
    the one with a field site (along its spins) stays, the other flips by the coin of its smallest site index."""
    if tile:
        monkeypatch.setenv("TSU_SW3D_TILE", tile)
    shape, per, T, seed = (4, 4, 8), (False, True, True), 1e-3, 21
    jr, jd, jl = (np.ones(shape, np.float32) for _ in range(3))
    jl[1] = 0.0
    jl[3] = 0.0
    for field_slab in (0, 1):
        h = np.zeros(shape, np.float32)
        h[2 * field_slab + 1, 3, 5] = 5.0
        free = 1 - field_slab
        root = 2 * free * shape[1] * shape[2]  # the free slab's smallest site index
        lat = hip.Lattice3D(*shape, per)
        try:
            lat.fill(1)
            lat.set_disorder(jr, jd, jl, h)
            want_free, flips = 1, 0
            for t in range(8):
                lat.cluster_sweep_field(T, 1, seed, t)
                s = lat.get_spins()
                if twin.flip_of_roots(np.array([root]), shape[2], seed, t)[0]:
                    want_free, flips = -want_free, flips + 1
                assert (s[2 * field_slab:2 * field_slab + 2] == 1).all(), f"the slab with the field changed at step {t}"
                assert (s[2 * free:2 * free + 2] == want_free).all(), f"the free slab at step {t}"
            assert flips > 0
        finally:
            lat.close()


def test_batch(hip):
    shape, per = (3, 6, 10), (False, True, True)
    kinds = ["gauss", "pmJ", "ferro+", "ferro-", "gauss"]
    dis = [_disorder(kinds[i], shape, per, 20 + i)[0] for i in range(5)]
    Ts = np.linspace(1.5, 4.0, 5)
    lats = [hip.Lattice3D(*shape, per) for _ in range(5)]
    serial = [hip.Lattice3D(*shape, per) for _ in range(5)]
    odd = hip.Lattice3D(3, 4, 6, False)
    try:
        for i in range(5):
            for l in (lats[i], serial[i]):
                l.randomize(100 + i)
                l.set_disorder(*dis[i])
        starts = [l.get_spins() for l in lats]
        hip.cluster_sweep_field_batch_3d(lats, 4, Ts, [7 + i for i in range(5)], [3 * i for i in range(5)], list(range(5)))
        for i in range(5):
            serial[i].cluster_sweep_field(Ts[i], 4, 7 + i, 3 * i, i)
            assert lats[i].cluster_launch_count() == 1 and lats[i].launch_count() == 0  # one launch for the five
            got = lats[i].get_spins()
            _same(got, serial[i].get_spins(), f"batch lattice {i} against the serial call")
            _same(got, twin.sweep(starts[i], per, *dis[i], Ts[i], 4, 7 + i, 3 * i, i), f"batch lattice {i}")
        # two shapes: one call per lattice, the same spins
        do, To = _disorder("gauss", (3, 4, 6), False, 2)
        odd.fill(1)
        odd.set_disorder(*do)
        before = lats[0].get_spins()
        hip.cluster_sweep_field_batch_3d([lats[0], odd], 2, [2.0, To], [1, 2], [0, 0])
        _same(odd.get_spins(), twin.sweep(np.ones((3, 4, 6), np.int8), False, *do, To, 2, 2, 0), "mixed batch")
        _same(lats[0].get_spins(), twin.sweep(before, per, *dis[0], 2.0, 2, 1, 0), "mixed batch, first lattice")
        assert lats[0].cluster_launch_count() == 2 and odd.cluster_launch_count() == 1
        with pytest.raises(ValueError, match="twice"):
            hip.cluster_sweep_field_batch_3d([odd, odd], 1, [2.0, 2.0], [1, 2], [0, 0])
        with pytest.raises(ValueError, match="Temperature must be positive"):
            hip.cluster_sweep_field_batch_3d([odd], 1, [0.0], [1], [0])
        assert odd.cluster_launch_count() == 1
    finally:
        for l in lats + serial + [odd]:
            l.close()


def test_errors_are_those_of_the_zero_field_call(hip, monkeypatch):
    shape = (4, 6, 8)
    d, _ = _disorder("gauss", shape, False, 1)
    lat = hip.Lattice3D(*shape, False)
    try:
        lat.fill(1)
        with pytest.raises(ValueError, match="set_disorder first"):
            lat.cluster_sweep_field(2.0, 1, 1, 0)
        lat.set_disorder(*d)
        with pytest.raises(hip.UnsupportedError, match="ghost spin"):
            lat.cluster_sweep(2.0, 1, 1, 0)  # the zero-field entry point refuses the field as before
        for T in (0.0, -1.0):
            with pytest.raises(ValueError, match="Temperature must be positive"):
                lat.cluster_sweep_field(T, 1, 1, 0)
        with pytest.raises(ValueError):
            lat.cluster_sweep_field(2.0, -1, 1, 0)
        monkeypatch.setenv("TSU_SW3D_TILE", "4x4x3")
        with pytest.raises(ValueError, match="even width"):
            lat.cluster_sweep_field(2.0, 1, 1, 0)
        monkeypatch.delenv("TSU_SW3D_TILE")
        lat.cluster_sweep_field(2.0, 0, 1, 0)
        assert (lat.get_spins() == 1).all() and lat.cluster_launch_count() == 0
    finally:
        lat.close()


ENUM = {(2, 2, 2): (20000, 4), (2, 3, 2): (50000, 8)}


@pytest.mark.parametrize("shape,T,seed,dseed", [((2, 2, 2), 2.0, 11, 3), ((2, 3, 2), 1.5, 13, 5)])
def test_exact_enumeration(hip, shape, T, seed, dseed):
    """The step samples exp(-E / T) / Z of E = -sum J s s' - sum h s: open lattices from all up, the couplings AND the Gaussian field
    of lattice3d_twin.enumeration_disorder; 100 steps discarded, then 20 000 states every 4 steps (2 x 2 x 2) or 50 000 every 8 steps
    (2 x 3 x 2; 88 % of its sites are frozen in a step, so its states decorrelate slowly: thinned to every 2 steps the twin itself
    gives p < 0.001) with the step counter running on; chi^2 of the state histogram over the states with expected count >= 5, the
    rest pooled.  The NumPy twin (bit-identical to the device) gives at these seeds chi^2 = 130.7 on 129 d.o.f. (p = 0.44, pooled
    0.81 %) and 275.2 on 296 d.o.f. (p = 0.80, pooled 1.99 %)."""
    n_samples, every = ENUM[shape]
    d = lat3.enumeration_disorder(shape, dseed)
    lat = hip.Lattice3D(*shape, False)
    try:
        lat.fill(1)
        lat.set_disorder(*d)
        lat.cluster_sweep_field(T, 100, seed, 0)
        want = twin.sweep(np.ones(shape, np.int8), False, *d, T, 100, seed, 0)
        _same(lat.get_spins(), want, f"enumeration {shape}: burn-in")
        codes, steps = [], 100
        for k in range(n_samples):
            lat.cluster_sweep_field(T, every, seed, steps)
            steps += every
            s = lat.get_spins()
            if k < 50:
                want = twin.sweep(want, False, *d, T, every, seed, steps - every)
                _same(s, want, f"enumeration {shape}: state {k}")
            codes.append(lat3.state_code(s))
    finally:
        lat.close()
    chi2, dof, p, pooled = lat3.boltzmann_chi2(codes, shape, d, T)
    print(f"\n{shape} T = {T}: chi2 = {chi2:.1f} on {dof} d.o.f., p = {p:.3f}, pooled share {pooled:.2%}")
    assert p >= 0.01, (chi2, dof, p)
    assert pooled <= 0.05, pooled


def _bimodal_field():
    return np.random.default_rng(7).choice(np.array([-1.0, 1.0], np.float32), size=(16, 16, 16))


@pytest.mark.parametrize("case,T", [("uniform", TC3), ("bimodal", 5.0)])
def test_equilibrium_at_16_cubed_against_heat_bath(hip, case, T):
    """Periodic 16^3, J = 1, in a uniform field h = 0.05 at T_c and in a bimodal field h_i = +-1 at T = 5: <E> / N and the signed
    <m> from ghost-spin steps and from k8_sweep, 20 batch means each, within 4 combined batch-means errors (the rule of the
    zero-field test)."""
    from tsu.models.ising import IsingModel3D
    n_batches, per = 20, 100
    kw = {"external_field": 0.05} if case == "uniform" else {"field": _bimodal_field()}

    def series(advance, burn):
        m = IsingModel3D(16, temperature=T, seed=31, initial="up", **kw)
        advance(m, burn)
        E, M = np.zeros((n_batches, per)), np.zeros((n_batches, per))
        for b in range(n_batches):
            for k in range(per):
                advance(m, 1)
                E[b, k] = m.energy() / m.n_spins
                M[b, k] = m.magnetization()
        e_b, m_b = E.mean(axis=1), M.mean(axis=1)
        return (e_b.mean(), e_b.std(ddof=1) / math.sqrt(n_batches), m_b.mean(), m_b.std(ddof=1) / math.sqrt(n_batches))

    e_sw, de_sw, m_sw, dm_sw = series(lambda m, n: m.ghost_cluster_update(n), 200)
    e_hb, de_hb, m_hb, dm_hb = series(lambda m, n: m.gibbs_update(10 * n), 100)
    print(f"\n16^3 {case} field, T = {T}: E/N ghost SW {e_sw:.5f} +- {de_sw:.5f}, heat-bath {e_hb:.5f} +- {de_hb:.5f}; "
          f"m ghost SW {m_sw:.5f} +- {dm_sw:.5f}, heat-bath {m_hb:.5f} +- {dm_hb:.5f}")
    assert abs(e_sw - e_hb) < 4 * math.hypot(de_sw, de_hb), (e_sw, e_hb, de_sw, de_hb)
    assert abs(m_sw - m_hb) < 4 * math.hypot(dm_sw, dm_hb), (m_sw, m_hb, dm_sw, dm_hb)


def test_ghost_cluster_update_counts_and_interleaves(hip):
    from tsu.models.ising import IsingModel3D
    shape, per, T, seed = (6, 8, 12), (True, False, True), 2.2, 4242
    d, _ = _disorder("gauss", shape, per, 8)
    j, h = d[:3], d[3]
    m = IsingModel3D(shape, temperature=T, periodic=per, seed=seed, initial="up", couplings=j, field=h)
    s = np.ones(shape, np.int8)
    m.gibbs_update(3)
    s = lat3.sweep(s, per, *j, h, T, 3, seed, 0)
    m.ghost_cluster_update(4)
    s = twin.sweep(s, per, *j, h, T, 4, seed, 0)
    assert m.sweep_count == 3 and m.cluster_count == 4  # the cluster counter only
    m.gibbs_update(2)
    s = lat3.sweep(s, per, *j, h, T, 2, seed, 3)
    _same(m.spins, s, "interleaved with heat-bath sweeps")
    m.equilibrate(n_sweeps=2, algorithm="swendsen_wang_ghost")
    s = twin.sweep(s, per, *j, h, T, 2, seed, 4)
    _same(m.spins, s, "equilibrate(swendsen_wang_ghost)")
    assert m.cluster_count == 6 and m.sweep_count == 5
    with pytest.raises(hip.UnsupportedError, match="ghost spin"):
        m.cluster_update(1)
    with pytest.raises(hip.UnsupportedError, match="ghost spin"):
        m.equilibrate(n_sweeps=1, algorithm="swendsen_wang")
    # without the field the two kinds of cluster step share one counter and one stream
    m.set_disorder(couplings=j, field=None)
    m.cluster_update(2)
    s = twin0.sweep(s, per, *j, T, 2, seed, 6)
    m.ghost_cluster_update(2)
    s = twin0.sweep(s, per, *j, T, 2, seed, 8)
    _same(m.spins, s, "zero field: cluster_update then ghost_cluster_update")
    assert m.cluster_count == 10 and m.sweep_count == 5
    assert m._lat.launch_count() == 10 and m._lat.cluster_launch_count() == 4


def test_temperature_scan_ghost_batch_equals_serial(hip):
    from tsu.models.ising import IsingModel3D, temperature_scan_3d
    temps = [3.5, 4.0, 4.5115, 5.5]
    shape = (6, 8, 12)
    h = np.random.default_rng(3).normal(scale=0.5, size=shape)
    out = temperature_scan_3d(shape, temps, n_equilibrate=10, n_measure=6, measure_every=3, seed=5, field=h,
                              algorithm="swendsen_wang_ghost", replicas=2)
    for i, T in enumerate(temps):
        m = IsingModel3D(shape, temperature=T, seed=5 + i, initial="up", field=h)
        m2 = IsingModel3D(shape, temperature=T, seed=5 + len(temps) + i, initial="up", field=h)
        m.ghost_cluster_update(10)
        m2.ghost_cluster_update(10)
        Ms, Es, Qs = [], [], []
        for _ in range(6):
            m.ghost_cluster_update(3)
            m2.ghost_cluster_update(3)
            Ms.append(m.magnetization())
            Es.append(m.energy())
            Qs.append(m.overlap(m2))
        Ms, Es, Qs = np.array(Ms), np.array(Es), np.array(Qs)
        assert out["magnetization"][i] == np.mean(np.abs(Ms))
        assert out["energy"][i] == np.mean(Es) / m.n_spins
        assert out["susceptibility"][i] == (np.mean(Ms ** 2) - np.mean(np.abs(Ms)) ** 2) * m.n_spins / T
        assert out["specific_heat"][i] == (np.mean(Es ** 2) - np.mean(Es) ** 2) / (T ** 2 * m.n_spins)
        assert out["overlap"][i] == np.mean(np.abs(Qs))
        assert out["overlap_sq"][i] == np.mean(Qs ** 2)
        assert m.sweep_count == 0 and m.cluster_count == 28
    assert sorted(out) == sorted(["temperatures", "magnetization", "energy", "susceptibility", "specific_heat", "overlap",
                                  "overlap_sq", "binder"])
    # external_field= is the constant-array case
    a = temperature_scan_3d(shape, temps[:2], n_equilibrate=4, n_measure=3, measure_every=2, seed=5, external_field=0.25,
                            algorithm="swendsen_wang_ghost")
    b = temperature_scan_3d(shape, temps[:2], n_equilibrate=4, n_measure=3, measure_every=2, seed=5, field=np.full(shape, 0.25),
                            algorithm="swendsen_wang_ghost")
    assert all((a[k] == b[k]).all() for k in a)
    # the default and the zero-field Swendsen-Wang scans are what they were; a field is still refused there
    g = temperature_scan_3d(shape, temps[:2], n_equilibrate=4, n_measure=3, measure_every=2, seed=5)
    z = temperature_scan_3d(shape, temps[:2], n_equilibrate=4, n_measure=3, measure_every=2, seed=5, algorithm="swendsen_wang")
    z2 = temperature_scan_3d(shape, temps[:2], n_equilibrate=4, n_measure=3, measure_every=2, seed=5, algorithm="swendsen_wang_ghost")
    for i, T in enumerate(temps[:2]):
        m = IsingModel3D(shape, temperature=T, seed=5 + i, initial="up")
        c = IsingModel3D(shape, temperature=T, seed=5 + i, initial="up")
        m.gibbs_update(4)
        c.cluster_update(4)
        Ms, Cs = [], []
        for _ in range(3):
            m.gibbs_update(2)
            c.cluster_update(2)
            Ms.append(m.magnetization())
            Cs.append(c.magnetization())
        assert g["magnetization"][i] == np.mean(np.abs(Ms))
        assert z["magnetization"][i] == z2["magnetization"][i] == np.mean(np.abs(Cs))
    with pytest.raises(hip.UnsupportedError, match="ghost spin"):
        temperature_scan_3d(shape, temps[:2], field=h, algorithm="swendsen_wang")

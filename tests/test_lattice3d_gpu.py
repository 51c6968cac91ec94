"""K8 heat-bath sweeps of 3-D disordered lattices on the GPU (csrc/ising3d.hip): bit-exact against the NumPy twin
(tests/helpers/lattice3d_twin.py) on periodic, open and mixed shapes, three kinds of disorder and four temperatures, split calls
and replicas; near-tie fields that push the decisions through the float64 branch (with and without couplings); D = 1 against K7
on the device; the energy, the sum of spins and the overlap; exact enumeration of two small open lattices; the +-J cube against
the K5 CSR route; the Python API."""
import importlib.util
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("lattice3d_twin", os.path.join(HERE, "helpers", "lattice3d_twin.py"))
twin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(twin)


@pytest.fixture(scope="module")
def hip():
    from tsu import _hip
    return _hip


def _disorder(kind, shape, periodic, seed):
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        jr, jd, jl, h = (rng.normal(size=shape) for _ in range(4))
    elif kind == "pmJ":
        jr, jd, jl = (np.where(rng.random(shape) < 0.5, 1.0, -1.0) for _ in range(3))
        h = None
    else:  # uniform J, Gaussian h (random-field)
        jr, jd, jl = (np.ones(shape) for _ in range(3))
        h = rng.normal(scale=0.7, size=shape)
    jr, jd, jl = (a.astype(np.float32) for a in (jr, jd, jl))
    pz, pr, pc = twin.axes(periodic)
    if not pc:
        jr[:, :, -1] = 0.0
    if not pr:
        jd[:, -1, :] = 0.0
    if not pz:
        jl[-1, :, :] = 0.0
    return jr, jd, jl, (None if h is None else h.astype(np.float32))


def _same(got, want, what):
    assert (got == want).all(), f"{what}: {int((got != want).sum())} sites differ, first {np.argwhere(got != want)[:4].tolist()}"


def _check(hip, shape, periodic, kind, T, calls, seed=5, replica=0):
    d = _disorder(kind, shape, periodic, seed + shape[0] * 13 + shape[1] * 7 + shape[2])
    lat = hip.Lattice3D(*shape, periodic)
    try:
        lat.randomize(seed + 1)
        lat.set_disorder(*d)
        want = lat.get_spins()
        for sweep0, n in calls:
            lat.sweep(T, n, seed, sweep0, replica)
            want = twin.sweep(want, periodic, *d, T, n, seed, sweep0, replica)
            _same(lat.get_spins(), want, f"{shape} periodic={periodic} {kind} T={T} sweep0={sweep0}")
        return lat, want, d
    except BaseException:
        lat.close()
        raise


SHAPES = [((4, 4, 4), True), ((4, 6, 40), True), ((6, 8, 1000), True), ((64, 64, 64), True), ((1, 9, 1), False),
          ((3, 5, 37), False), ((5, 1, 53), False), ((2, 2, 2), False), ((4, 37, 64), (True, False, True)),
          ((7, 6, 40), (False, True, True))]


@pytest.mark.parametrize("shape,periodic", SHAPES)
@pytest.mark.parametrize("kind", ["gauss", "pmJ", "rfim"])
@pytest.mark.parametrize("T", [0.4, 1.1, 2.27, 5.0])
def test_twin_parity(hip, shape, periodic, kind, T):
    lat, _, _ = _check(hip, shape, periodic, kind, T, [(0, 3), (3, 5)])
    assert lat.launch_count() == 16  # one launch per half-sweep
    lat.close()


def test_twin_parity_large(hip):
    lat, _, _ = _check(hip, (256, 256, 64), True, "gauss", 1.1, [(0, 3), (3, 5)])
    lat.close()


def test_randomize_is_the_2d_stream_reshaped_and_fill(hip):
    for shape in ((3, 5, 37), (4, 6, 40), (2, 3, 1000)):
        a = hip.Lattice3D(*shape, False)
        b = hip.Lattice(shape[0] * shape[1], shape[2], False)
        try:
            a.randomize(77, 3)
            b.randomize(77, 3)
            s = a.get_spins()
            assert (s == b.get_spins().reshape(shape)).all() and set(np.unique(s)) == {-1, 1}
            assert a.sum_spins() == int(s.sum(dtype=np.int64))
            a.fill(-1)
            assert (a.get_spins() == -1).all() and a.sum_spins() == -int(np.prod(shape))
            with pytest.raises(ValueError):
                a.fill(0)
        finally:
            a.close()
            b.close()


def test_split_calls_equal_one_call_and_replica_changes_the_stream(hip):
    shape, per, T = (6, 8, 40), True, 1.1
    d = _disorder("gauss", shape, per, 21)
    out = []
    for calls, replica in (([(0, 8)], 0), ([(0, 1), (1, 4), (5, 3)], 0), ([(0, 8)], 1)):
        lat = hip.Lattice3D(*shape, per)
        lat.randomize(9)
        lat.set_disorder(*d)
        for sweep0, n in calls:
            lat.sweep(T, n, 17, sweep0, replica)
        out.append(lat.get_spins())
        lat.close()
    assert (out[0] == out[1]).all()
    assert (out[0] != out[2]).any()


@pytest.mark.parametrize("shape,periodic", [((64, 64, 64), True), ((3, 5, 37), False)])
@pytest.mark.parametrize("T", [0.4, 2.27])
def test_near_ties(hip, shape, periodic, T):
    """h = fp32(T / 2 logit(u)) with all J = 0: every decision of sweep 0 sits on its threshold (within fp32 rounding of h), far
    inside the screen's margin, so the float64 branch and the lo16 block decide."""
    seed = 9
    h = twin.tie_field(shape, T, seed)
    z = np.zeros(shape, np.float32)
    start = np.ones(shape, np.int8)
    stats = {}
    want = twin.sweep(start, periodic, z, z, z, h, T, 1, seed, 0, 0, stats=stats)
    assert stats["near"] > 0.9 * stats["sites"], stats
    lat = hip.Lattice3D(*shape, periodic)
    try:
        lat.set_spins(start)
        lat.set_disorder(z, z, z, h)
        lat.sweep(T, 1, seed, 0)
        _same(lat.get_spins(), want, f"near ties {shape} T={T}")
        want = twin.sweep(want, periodic, z, z, z, h, T, 2, seed, 1)
        lat.sweep(T, 2, seed, 1)
        _same(lat.get_spins(), want, f"after near ties {shape} T={T}")
    finally:
        lat.close()


@pytest.mark.parametrize("shape,periodic,T", [((64, 64, 64), True, 1.1), ((8, 6, 40), (False, True, True), 0.4),
                                              ((3, 5, 37), False, 2.27)])
def test_near_ties_of_seven_term_sums(hip, shape, periodic, T):
    """Gaussian couplings and the tie field computed for the actual start state: the seven-term sums, not only h, sit on the
    thresholds (colour 1's after the colour-0 half-sweep).  This is what guards the screen's margin for six additions."""
    seed = 12
    jr, jd, jl, _ = _disorder("gauss", shape, periodic, 31)
    start = np.where(np.random.default_rng(2).random(shape) < 0.5, 1, -1).astype(np.int8)
    h = twin.tie_field(shape, T, seed, 0, spins=start, periodic=periodic, couplings=(jr, jd, jl))
    stats = {}
    want = twin.sweep(start, periodic, jr, jd, jl, h, T, 1, seed, 0, 0, stats=stats)
    assert stats["near"] > 0.9 * stats["sites"], stats
    lat = hip.Lattice3D(*shape, periodic)
    try:
        lat.set_spins(start)
        lat.set_disorder(jr, jd, jl, h)
        lat.sweep(T, 1, seed, 0)
        _same(lat.get_spins(), want, f"seven-term near ties {shape} T={T}")
    finally:
        lat.close()


@pytest.mark.parametrize("rows,cols,periodic", [(6, 40, True), (128, 1000, True), (37, 53, False)])
def test_one_layer_equals_k7_on_the_device(hip, rows, cols, periodic):
    rng = np.random.default_rng(rows)
    jr, jd, h = (rng.normal(size=(rows, cols)).astype(np.float32) for _ in range(3))
    if not periodic:
        jr[:, -1] = 0.0
        jd[-1, :] = 0.0
    shape = (1, rows, cols)
    a = hip.Lattice3D(1, rows, cols, (False, periodic, periodic))
    b = hip.Lattice(rows, cols, periodic)
    try:
        a.randomize(4, 1)
        b.randomize(4, 1)
        a.set_disorder(jr.reshape(shape), jd.reshape(shape), np.zeros(shape, np.float32), h.reshape(shape))
        b.set_disorder(jr, jd, h)
        for T, n, sweep0, replica in ((1.3, 3, 0, 0), (0.4, 5, 3, 2)):
            a.sweep(T, n, 23, sweep0, replica)
            b.disorder_sweep(T, n, 23, sweep0, replica)
            _same(a.get_spins().reshape(rows, cols), b.get_spins(), f"D = 1 against K7, {rows}x{cols} periodic={periodic} T={T}")
        assert a.energy() == pytest.approx(b.disorder_energy(), rel=1e-12)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("shape,periodic", [((4, 6, 40), True), ((64, 64, 64), True), ((3, 5, 37), False),
                                            ((4, 37, 64), (True, False, True)), ((6, 8, 1000), True)])
def test_energy_sum_and_overlap(hip, shape, periodic):
    lat, s, d = _check(hip, shape, periodic, "gauss", 1.1, [(0, 2)])
    other = hip.Lattice3D(*shape, periodic)
    try:
        want, total = twin.energy_terms(s, periodic, *d)
        e = lat.energy()
        assert abs(e - want) <= 1e-12 * total, (e, want, total)
        assert lat.energy() == e  # the same bits on every call
        assert lat.sum_spins() == int(s.sum(dtype=np.int64))
        other.randomize(99)
        t = other.get_spins()
        assert lat.overlap(other) == twin.overlap(s, t) and other.overlap(lat) == twin.overlap(s, t)
        assert lat.overlap(lat) == int(np.prod(shape))
        # +-J couplings with a dyadic field: every partial sum is an exactly representable number
        rng = np.random.default_rng(3)
        jr, jd, jl, _ = _disorder("pmJ", shape, periodic, 8)
        h = (rng.integers(-8, 9, size=shape) / 4.0).astype(np.float32)
        lat.set_disorder(jr, jd, jl, h)
        assert lat.energy() == twin.energy(s, periodic, jr, jd, jl, h)
        lat.set_disorder(jr, jd, jl, None)
        assert lat.energy() == twin.energy(s, periodic, jr, jd, jl)
    finally:
        lat.close()
        other.close()


def test_handle_validation(hip):
    with pytest.raises(hip.UnsupportedError):
        hip.Lattice3D(4, 6, 2, True)
    with pytest.raises(hip.UnsupportedError):
        hip.Lattice3D(5, 6, 8, (True, False, False))
    with pytest.raises(ValueError):
        hip.Lattice3D(0, 6, 8, False)
    lat = hip.Lattice3D(3, 4, 5, (False, True, False))
    other = hip.Lattice3D(3, 4, 6, False)
    try:
        jr, jd, jl, h = twin.uniform_disorder((3, 4, 5), (False, True, False), 1.0, 0.5)
        with pytest.raises(ValueError, match="set_disorder first"):
            lat.sweep(1.0, 1, 0)
        with pytest.raises(ValueError, match="set_disorder first"):
            lat.energy()
        for k, name in ((0, "last column"), (2, "last layer")):
            bad = [jr.copy(), jd.copy(), jl.copy()]
            bad[k][(-1, 1, -1)] = 0.25
            with pytest.raises(ValueError, match=name):
                lat.set_disorder(*bad, h)
        bad = h.copy()
        bad[1, 2, 3] = np.nan
        with pytest.raises(ValueError, match="non-finite"):
            lat.set_disorder(jr, jd, jl, bad)
        lat.set_disorder(jr, jd, jl, h)
        for T in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="Temperature must be positive"):
                lat.sweep(T, 1, 0)
        with pytest.raises(ValueError):
            lat.sweep(1.0, -1, 0)
        with pytest.raises(ValueError, match="shapes differ"):
            lat.overlap(other)
        lat.sweep(1.0, 0, 0)
        assert lat.launch_count() == 0
    finally:
        lat.close()
        other.close()


@pytest.mark.parametrize("shape,T,seed,dseed", [((2, 2, 2), 2.0, 11, 3), ((2, 3, 2), 1.5, 13, 5)])
def test_exact_enumeration(hip, shape, T, seed, dseed):
    """The rule samples exp(-E / T) / Z: 100 sweeps discarded, then 20 000 states taken every 4 sweeps with the sweep counter running
    on; chi^2 of the state histogram over the states with expected count >= 5, the rest pooled.  The NumPy twin (bit-identical
    to the device) gives chi^2 = 134.7 on 129 d.o.f. (p = 0.35, pooled 0.8 %) and 171.9 on 186 d.o.f. (p = 0.76, pooled 3.9 %)."""
    d = twin.enumeration_disorder(shape, dseed)
    lat = hip.Lattice3D(*shape, False)
    try:
        lat.fill(1)
        lat.set_disorder(*d)
        lat.sweep(T, 100, seed, 0, 0)
        # the device against the twin over the discarded sweeps and the first recorded states
        want = twin.sweep(np.ones(shape, np.int8), False, *d, T, 100, seed, 0)
        _same(lat.get_spins(), want, f"enumeration {shape}: burn-in")
        codes, sweeps = [], 100
        for k in range(20000):
            lat.sweep(T, 4, seed, sweeps, 0)
            sweeps += 4
            s = lat.get_spins()
            if k < 50:
                want = twin.sweep(want, False, *d, T, 4, seed, sweeps - 4)
                _same(s, want, f"enumeration {shape}: state {k}")
            codes.append(twin.state_code(s))
    finally:
        lat.close()
    chi2, dof, p, pooled = twin.boltzmann_chi2(codes, shape, d, T)
    print(f"{shape} T = {T}: chi2 = {chi2:.1f} on {dof} d.o.f., p = {p:.3f}, pooled share {pooled:.2%}")
    assert p >= 0.01, (chi2, dof, p)
    assert pooled <= 0.05, pooled


def test_pmj_cube_against_k5_route(hip):
    """8 x 8 x 8 periodic +-J at T = 2.0 against the CSR gather kernel on the same couplings (independent code, another random
    stream): <E> / N from 20 batch means each, within 4 combined standard errors."""
    import scipy.sparse as sp
    from tsu.models.ising import IsingConfig, IsingModel, IsingModel3D
    L, T = 8, 2.0
    shape = (L, L, L)
    jr, jd, jl, _ = _disorder("pmJ", shape, True, 77)
    idx = np.arange(L ** 3).reshape(shape)
    rows = np.concatenate([idx.ravel()] * 3)
    cols = np.concatenate([np.roll(idx, -1, axis=2).ravel(), np.roll(idx, -1, axis=1).ravel(), np.roll(idx, -1, axis=0).ravel()])
    vals = np.concatenate([jr.ravel(), jd.ravel(), jl.ravel()]).astype(np.float64)
    J = sp.coo_matrix((vals, (rows, cols)), shape=(L ** 3, L ** 3))
    J = (J + J.T).tocsr()
    n_batches, per = 20, 100
    m = IsingModel3D(shape, temperature=T, seed=3, couplings=(jr, jd, jl))
    try:
        m.gibbs_update(2000)
        E8 = np.zeros((n_batches, per))
        for bi in range(n_batches):
            for j in range(per):
                m.gibbs_update(5)
                E8[bi, j] = m.energy() / m.n_spins
    finally:
        m._lat.close()
    # K5 draws its Philox seed and start state from np.random: pinned here so that the comparison is the same on every run
    state = np.random.get_state()
    np.random.seed(20261016)
    try:
        g = IsingModel(L ** 3, IsingConfig(temperature=T, n_burnin=2000, n_sweeps=5), bias_mode="physical", graph="sparse")
        g.J = J
        samples = g.sample(n_batches * per)
    finally:
        np.random.set_state(state)
    E5 = np.array([g.energy(s) for s in samples]).reshape(n_batches, per) / L ** 3
    # the twin's energy of a K5 sample agrees with IsingModel.energy (same Hamiltonian)
    assert twin.energy(samples[-1].reshape(shape), True, jr, jd, jl) == pytest.approx(g.energy(samples[-1]), rel=1e-12)
    b8, b5 = E8.mean(axis=1), E5.mean(axis=1)
    se = math.sqrt(b8.var(ddof=1) / n_batches + b5.var(ddof=1) / n_batches)
    print(f"K8 <E>/N = {b8.mean():.5f}, K5 <E>/N = {b5.mean():.5f}, combined s.e. {se:.5f}")
    assert abs(b8.mean() - b5.mean()) < 4 * se, (b8.mean(), b5.mean(), se)


def test_api(hip):
    from tsu.models.ising import IsingModel3D, temperature_scan_3d
    rng = np.random.default_rng(2)
    shape, per = (4, 6, 8), (True, True, False)
    jr, jd, jl, _ = _disorder("pmJ", shape, per, 5)
    h = rng.normal(size=shape)
    m = IsingModel3D(shape, temperature=1.5, periodic=per, seed=4, couplings=(jr, jd, jl))
    lat = hip.Lattice3D(*shape, per)
    try:
        lat.randomize(4)
        lat.set_disorder(jr, jd, jl)
        assert (m.spins == lat.get_spins()).all() and m.disorder[3] is None
        m.gibbs_update(3)
        lat.sweep(1.5, 3, 4, 0)
        s = m.spins
        assert (s == lat.get_spins()).all()
        assert m.energy() == lat.energy() and m.magnetization() == lat.sum_spins() / 192
        m.set_disorder(couplings=(jr, jd, jl), field=h)
        assert (m.spins == s).all() and m.sweep_count == 3
        d = m.disorder
        assert d[3].dtype == np.float32 and (d[3] == h.astype(np.float32)).all() and (d[0] == jr).all()
        m.equilibrate(2.5, n_sweeps=4)
        assert m.sweep_count == 7 and m.temperature == 2.5
        want = twin.sweep(s, per, jr, jd, jl, h.astype(np.float32), 2.5, 4, 4, 3)
        assert (m.spins == want).all()
        m.spins = -want
        assert (m.spins == -want).all() and m.overlap(m) == 1.0
        with pytest.raises(ValueError):
            m.spins = np.zeros(shape)
        with pytest.raises(ValueError):
            m.equilibrate(0.0)
    finally:
        m._lat.close()
        lat.close()

    # a scan equals its models run one after another; replicas=2 overlaps equal those from the spins
    Ts = [1.0, 2.0, 3.5]
    N = 192
    hh = h.astype(np.float32)
    kw = dict(n_equilibrate=20, n_measure=6, measure_every=3, seed=100, initial="random", periodic=per)
    out = temperature_scan_3d(shape, Ts, couplings=(jr, jd, jl), field=hh, replicas=2, **kw)
    Q = np.zeros((len(Ts), 6))
    for i, T in enumerate(Ts):
        a = IsingModel3D(shape, temperature=T, periodic=per, seed=100 + i, couplings=(jr, jd, jl), field=hh)
        b = IsingModel3D(shape, temperature=T, periodic=per, seed=100 + len(Ts) + i, couplings=(jr, jd, jl), field=hh)
        a.gibbs_update(20)
        b.gibbs_update(20)
        E, M = [], []
        for j in range(6):
            a.gibbs_update(3)
            b.gibbs_update(3)
            sa, sb = a.spins, b.spins
            E.append(twin.energy(sa, per, jr, jd, jl, hh))
            M.append(sa.sum() / N)
            Q[i, j] = twin.overlap(sa, sb) / N
        a._lat.close()
        b._lat.close()
        E, M = np.array(E), np.array(M)
        assert out["energy"][i] == pytest.approx(E.mean() / N, rel=1e-12, abs=1e-12)
        assert out["magnetization"][i] == np.mean(np.abs(M))
    assert np.array_equal(out["overlap"], np.mean(np.abs(Q), axis=1))
    assert np.array_equal(out["overlap_sq"], np.mean(Q ** 2, axis=1))
    assert np.allclose(out["binder"], 0.5 * (3 - np.mean(Q ** 4, axis=1) / np.mean(Q ** 2, axis=1) ** 2))
    one = temperature_scan_3d(shape, Ts, couplings=(jr, jd, jl), field=hh, **kw)
    assert "overlap" not in one
    for k in ("magnetization", "energy", "susceptibility", "specific_heat"):
        assert np.array_equal(one[k], out[k])


def test_uniform_ferromagnet_orders_below_and_disorders_above_tc(hip):
    """Uniform coupling = 1 on 16^3 periodic from all up, 300 sweeps: T = 3.0 and T = 6.0 are far from T_c = 4.5115 (the CPU twin
    with seed 1 gives m = 0.94 .. 0.96 and |m| <= 0.10 over the next 100 sweeps)."""
    from tsu.models.ising import IsingModel3D
    for T, ordered in ((3.0, True), (6.0, False)):
        m = IsingModel3D(16, coupling=1.0, temperature=T, seed=1, initial="up")
        try:
            m.gibbs_update(300)
            for _ in range(10):
                m.gibbs_update(10)
                mag = m.magnetization()
                assert (abs(mag) > 0.8) if ordered else (abs(mag) < 0.2), (T, mag)
        finally:
            m._lat.close()

"""K7 disordered heat-bath sweeps on the GPU (csrc/ising2d_disorder.hip): bit-exact against the NumPy twin
(tests/helpers/disorder_twin.py) on periodic and open shapes, three kinds of disorder and four temperatures, split calls and
replicas; near-tie fields that push the decisions through the float64 branch; constant dyadic arrays against K1 bit for bit;
the disordered energy and the overlap; the Mattis gauge against Onsager / Yang; ±J against the K5 CSR route; the Python API."""
import importlib.util
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("disorder_twin", os.path.join(HERE, "helpers", "disorder_twin.py"))
twin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(twin)

TC = 2.0 / math.log(1.0 + math.sqrt(2.0))


@pytest.fixture(scope="module")
def hip():
    from tsu import _hip
    return _hip


def _disorder(kind, rows, cols, periodic, seed):
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        jr, jd, h = (rng.normal(size=(rows, cols)) for _ in range(3))
    elif kind == "pmJ":
        jr, jd = (np.where(rng.random((rows, cols)) < 0.5, 1.0, -1.0) for _ in range(2))
        h = None
    else:  # uniform J, Gaussian h (random-field)
        jr, jd = np.ones((rows, cols)), np.ones((rows, cols))
        h = rng.normal(scale=0.7, size=(rows, cols))
    jr, jd = jr.astype(np.float32), jd.astype(np.float32)
    if not periodic:
        jr[:, -1] = 0.0
        jd[-1, :] = 0.0
    return jr, jd, (None if h is None else h.astype(np.float32))


def _check(hip, rows, cols, periodic, kind, T, calls, seed=5, replica=0):
    jr, jd, h = _disorder(kind, rows, cols, periodic, seed + rows * 7 + cols)
    lat = hip.Lattice(rows, cols, periodic)
    try:
        lat.randomize(seed + 1)
        lat.set_disorder(jr, jd, h)
        want = lat.get_spins()
        for sweep0, n in calls:
            lat.disorder_sweep(T, n, seed, sweep0, replica)
            want = twin.sweep(want, periodic, jr, jd, h, T, n, seed, sweep0, replica)
            got = lat.get_spins()
            assert (got == want).all(), f"{rows}x{cols} periodic={periodic} {kind} T={T} sweep0={sweep0}: " \
                                        f"{int((got != want).sum())} sites differ, first {np.argwhere(got != want)[:4].tolist()}"
        return lat, want, (jr, jd, h)
    except BaseException:
        lat.close()
        raise


SMALL = [(4, 4, True), (6, 10, True), (64, 64, True), (128, 1000, True), (1, 9, False), (9, 1, False), (37, 53, False),
         (513, 257, False)]


@pytest.mark.parametrize("rows,cols,periodic", SMALL)
@pytest.mark.parametrize("kind", ["gauss", "pmJ", "rfim"])
@pytest.mark.parametrize("T", [0.4, 1.0, 2.27, 5.0])
def test_twin_parity(hip, rows, cols, periodic, kind, T):
    lat, _, _ = _check(hip, rows, cols, periodic, kind, T, [(0, 3), (3, 5)])
    lat.close()


@pytest.mark.parametrize("kind", ["gauss", "pmJ", "rfim"])
def test_twin_parity_1000(hip, kind):
    lat, _, _ = _check(hip, 1000, 1000, True, kind, 2.27, [(0, 3), (3, 5)], seed=11)
    lat.close()


@pytest.mark.parametrize("rows,cols,periodic", [(6, 10, True), (37, 53, False), (128, 1000, True)])
def test_split_calls_equal_one_call_and_replicas(hip, rows, cols, periodic):
    jr, jd, h = _disorder("gauss", rows, cols, periodic, 3)
    outs = []
    for calls in ([(0, 8)], [(0, 3), (3, 5)]):
        lat = hip.Lattice(rows, cols, periodic)
        lat.randomize(9)
        lat.set_disorder(jr, jd, h)
        for sweep0, n in calls:
            lat.disorder_sweep(1.3, n, 21, sweep0, 5)
        outs.append(lat.get_spins())
        lat.close()
    assert (outs[0] == outs[1]).all()
    s0 = hip.Lattice(rows, cols, periodic)
    s0.randomize(9)
    start = s0.get_spins()
    s0.close()
    assert (outs[0] == twin.sweep(start, periodic, jr, jd, h, 1.3, 8, 21, 0, 5)).all()
    assert not (outs[0] == twin.sweep(start, periodic, jr, jd, h, 1.3, 8, 21, 0, 0)).all()  # the replica is in the stream


@pytest.mark.parametrize("rows,cols,periodic", [(64, 64, True), (128, 1000, True), (37, 53, False), (1, 9, False)])
@pytest.mark.parametrize("T", [0.4, 2.27])
def test_near_ties_go_through_the_exact_branch(hip, rows, cols, periodic, T):
    seed = 13
    h = twin.tie_field(rows, cols, T, seed)
    z = np.zeros((rows, cols), np.float32)
    lat = hip.Lattice(rows, cols, periodic)
    try:
        lat.fill(1)
        lat.set_disorder(z, z, h)
        stats = {}
        want = twin.sweep(np.ones((rows, cols), np.int8), periodic, z, z, h, T, 1, seed, 0, 0, stats=stats)
        assert stats["near"] > 0.9 * stats["sites"], stats
        lat.disorder_sweep(T, 1, seed, 0, 0)
        got = lat.get_spins()
        assert (got == want).all(), int((got != want).sum())
        if rows * cols >= 1000:
            assert 0.3 < (got > 0).mean() < 0.7
    finally:
        lat.close()


@pytest.mark.parametrize("rows,cols,periodic", [(512, 512, True), (4096, 4096, True), (333, 517, False)])
@pytest.mark.parametrize("J,h", [(1.0, 0.0), (0.5, 0.25), (-0.75, 0.5)])
@pytest.mark.parametrize("T", [TC, 1.5])
def test_uniform_arrays_equal_k1(hip, rows, cols, periodic, J, h, T):
    from tsu.models.ising import IsingModel2D
    jr, jd, hh = twin.uniform_disorder(rows, cols, periodic, J, h)
    k1 = IsingModel2D((rows, cols), coupling=J, external_field=h, temperature=T, periodic=periodic, seed=77)
    k7 = IsingModel2D((rows, cols), temperature=T, periodic=periodic, seed=77, couplings=(jr, jd), field=hh)
    try:
        k1.gibbs_update(16)
        k7.gibbs_update(16)
        assert k7._lat.disorder_launch_count() == 32 and k7._lat.launch_count() == 0
        a, b = k1.spins, k7.spins
        assert (a == b).all(), int((a != b).sum())
        assert k7.energy() == pytest.approx(k1.energy(), rel=1e-12, abs=1e-9)
        k7.clear_disorder()
        k7.coupling, k7.external_field = J, h
        k1.gibbs_update(3)
        k7.gibbs_update(3)
        assert k7._lat.launch_count() > 0
        assert (k1.spins == k7.spins).all()
    finally:
        k1._lat.close()
        k7._lat.close()


def test_full_size_4096_gaussian(hip):
    lat, want, (jr, jd, h) = _check(hip, 4096, 4096, True, "gauss", 2.27, [(0, 2)], seed=3)
    try:
        e = lat.disorder_energy()
        assert e == pytest.approx(twin.energy(want, True, jr, jd, h), rel=1e-12)
    finally:
        lat.close()


@pytest.mark.parametrize("rows,cols,periodic", [(6, 10, True), (37, 53, False), (1000, 1000, True), (513, 257, False)])
def test_energy_and_overlap(hip, rows, cols, periodic):
    from tsu.models.ising import IsingModel2D
    jr, jd, h = _disorder("gauss", rows, cols, periodic, 8)
    a = IsingModel2D((rows, cols), temperature=1.0, periodic=periodic, seed=1, couplings=(jr, jd), field=h)
    b = IsingModel2D((rows, cols), temperature=1.0, periodic=periodic, seed=2)
    try:
        a.gibbs_update(3)
        b.gibbs_update(2)
        sa, sb = a.spins, b.spins
        e = a.energy()
        assert e == pytest.approx(twin.energy(sa, periodic, jr, jd, h), rel=1e-12)
        assert all(a.energy() == e for _ in range(5))  # the same bits on every call
        q = twin.overlap(sa, sb)
        assert a._lat.overlap(b._lat) == q and b._lat.overlap(a._lat) == q
        assert a.overlap(b) == q / (rows * cols)
        assert a.overlap(a) == 1.0
    finally:
        a._lat.close()
        b._lat.close()


def _onsager_energy(T, J=1.0):
    from scipy.special import ellipk
    b = 1.0 / T
    k = 2.0 * math.sinh(2 * b * J) / math.cosh(2 * b * J) ** 2
    return -J / math.tanh(2 * b * J) * (1 + 2 / math.pi * (2 * math.tanh(2 * b * J) ** 2 - 1) * ellipk(k * k))


@pytest.mark.parametrize("T", [2.0, 3.0])
def test_mattis_gauge_onsager_and_yang(hip, T):
    from tsu.models.ising import IsingModel2D
    L = 256
    rng = np.random.default_rng(40)
    eps = np.where(rng.random((L, L)) < 0.5, 1, -1).astype(np.int8)
    jr = (eps * np.roll(eps, -1, axis=1)).astype(np.float32)
    jd = (eps * np.roll(eps, -1, axis=0)).astype(np.float32)
    m = IsingModel2D(L, temperature=T, seed=31, couplings=(jr, jd))
    ref = IsingModel2D(L, temperature=T, seed=32)
    try:
        m.spins = eps
        ref.spins = eps
        m.gibbs_update(500)
        n_batches, per = 20, 100
        E, M = np.zeros((n_batches, per)), np.zeros((n_batches, per))
        for bi in range(n_batches):
            for j in range(per):
                m.gibbs_update(2)
                E[bi, j] = m.energy() / m.n_spins
                M[bi, j] = abs(m.overlap(ref))
        e_b, m_b = E.mean(axis=1), M.mean(axis=1)
        e_se, m_se = e_b.std(ddof=1) / math.sqrt(n_batches), m_b.std(ddof=1) / math.sqrt(n_batches)
        e_exact = _onsager_energy(T)
        assert abs(e_b.mean() - e_exact) < 4 * e_se, (e_b.mean(), e_exact, e_se)
        if T < TC:
            m_exact = (1 - math.sinh(2 / T) ** -4) ** 0.125
            assert abs(m_b.mean() - m_exact) < 4 * m_se, (m_b.mean(), m_exact, m_se)
    finally:
        m._lat.close()
        ref._lat.close()


def test_edwards_anderson_against_k5_route(hip):
    import scipy.sparse as sp
    from tsu.models.ising import IsingConfig, IsingModel, IsingModel2D
    L, T = 32, 1.5
    jr, jd, _ = _disorder("pmJ", L, L, True, 77)
    idx = np.arange(L * L).reshape(L, L)
    rows = np.concatenate([idx.ravel(), idx.ravel()])
    cols = np.concatenate([np.roll(idx, -1, axis=1).ravel(), np.roll(idx, -1, axis=0).ravel()])
    vals = np.concatenate([jr.ravel(), jd.ravel()]).astype(np.float64)
    J = sp.coo_matrix((vals, (rows, cols)), shape=(L * L, L * L))
    J = (J + J.T).tocsr()
    n_batches, per = 20, 100
    # K7
    m = IsingModel2D(L, temperature=T, seed=3, couplings=(jr, jd))
    try:
        m.gibbs_update(2000)
        E7 = np.zeros((n_batches, per))
        for bi in range(n_batches):
            for j in range(per):
                m.gibbs_update(5)
                E7[bi, j] = m.energy() / m.n_spins
    finally:
        m._lat.close()
    # K5: the CSR gather kernel on the same couplings
    g = IsingModel(L * L, IsingConfig(temperature=T, n_burnin=2000, n_sweeps=5), bias_mode="physical", graph="sparse")
    g.J = J
    samples = g.sample(n_batches * per)
    E5 = np.array([g.energy(s) for s in samples]).reshape(n_batches, per) / (L * L)
    # the twin's energy of the K5 samples agrees with IsingModel.energy (same Hamiltonian)
    s_last = samples[-1].reshape(L, L)
    assert twin.energy(s_last, True, jr, jd) == pytest.approx(g.energy(samples[-1]), rel=1e-12)
    b7, b5 = E7.mean(axis=1), E5.mean(axis=1)
    se = math.sqrt(b7.var(ddof=1) / n_batches + b5.var(ddof=1) / n_batches)
    assert abs(b7.mean() - b5.mean()) < 4 * se, (b7.mean(), b5.mean(), se)


def test_api(hip):
    from tsu.models.ising import IsingModel2D, temperature_scan
    rng = np.random.default_rng(2)
    jr, jd = (np.where(rng.random((16, 16)) < 0.5, 1.0, -1.0).astype(np.float32) for _ in range(2))
    m = IsingModel2D(16, temperature=1.5, seed=4, couplings=(jr, jd))
    try:
        with pytest.raises(hip.UnsupportedError):
            m.cluster_update(1)
        with pytest.raises(hip.UnsupportedError):
            m.equilibrate(algorithm="swendsen_wang", n_sweeps=1)
        m.gibbs_update(3)
        s = m.spins
        h = rng.normal(size=(16, 16))
        m.set_disorder(couplings=(jr, jd), field=h)
        assert (m.spins == s).all() and m.sweep_count == 3
        d = m.disorder
        assert d[2].dtype == np.float32 and (d[2] == h.astype(np.float32)).all() and (d[0] == jr).all()
        m.equilibrate(n_sweeps=4)
        assert m.sweep_count == 7
        assert (m.spins == twin.sweep(s, True, jr, jd, h, 1.5, 4, 4, 3)).all()
        m.clear_disorder()
        assert m.disorder is None
        m.cluster_update(1)
    finally:
        m._lat.close()

    # a disordered scan equals its models run one after another; replicas=2 overlaps equal those from the spins
    Ts = [1.0, 2.0, 3.5]
    h = rng.normal(size=(16, 16)).astype(np.float32)
    kw = dict(n_equilibrate=20, n_measure=6, measure_every=3, seed=100, initial="random")
    out = temperature_scan(16, Ts, couplings=(jr, jd), field=h, replicas=2, **kw)
    Q = np.zeros((len(Ts), 6))
    for i, T in enumerate(Ts):
        a = IsingModel2D(16, temperature=T, seed=100 + i, initial="random", couplings=(jr, jd), field=h)
        b = IsingModel2D(16, temperature=T, seed=100 + len(Ts) + i, initial="random", couplings=(jr, jd), field=h)
        a.gibbs_update(20)
        b.gibbs_update(20)
        E, M = [], []
        for j in range(6):
            a.gibbs_update(3)
            b.gibbs_update(3)
            sa, sb = a.spins, b.spins
            E.append(twin.energy(sa, True, jr, jd, h))
            M.append(sa.sum() / 256)
            Q[i, j] = twin.overlap(sa, sb) / 256
        a._lat.close()
        b._lat.close()
        E, M = np.array(E), np.array(M)
        assert out["energy"][i] == pytest.approx(E.mean() / 256, rel=1e-12, abs=1e-12)
        assert out["magnetization"][i] == np.mean(np.abs(M))
    assert np.array_equal(out["overlap"], np.mean(np.abs(Q), axis=1))
    assert np.array_equal(out["overlap_sq"], np.mean(Q ** 2, axis=1))
    assert np.allclose(out["binder"], 0.5 * (3 - np.mean(Q ** 4, axis=1) / np.mean(Q ** 2, axis=1) ** 2))
    one = temperature_scan(16, Ts, couplings=(jr, jd), field=h, **kw)
    assert "overlap" not in one
    for k in ("magnetization", "energy", "susceptibility", "specific_heat"):
        assert np.array_equal(one[k], out[k])


def test_errors(hip):
    lat = hip.Lattice(8, 8, True)
    try:
        with pytest.raises(ValueError):
            lat.disorder_sweep(1.0, 1, 0)  # no disorder yet
        z = np.zeros((8, 8), np.float32)
        with pytest.raises(ValueError):
            lat.set_disorder(np.full((8, 8), np.nan, np.float32), z)
        lat.set_disorder(z, z)
        with pytest.raises(ValueError):
            lat.disorder_sweep(0.0, 1, 0)
        other = hip.Lattice(8, 6, True)
        with pytest.raises(ValueError):
            lat.overlap(other)
        other.close()
    finally:
        lat.close()
    lat = hip.Lattice(5, 7, False)
    try:
        jr = np.ones((5, 7), np.float32)
        with pytest.raises(ValueError, match="last column"):
            lat.set_disorder(jr, np.zeros((5, 7), np.float32))
    finally:
        lat.close()

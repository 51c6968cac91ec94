"""K7 parallel tempering on the GPU (tsu_pt2d_*, csrc/ising2d_disorder.hip): batched sweeps equal per-walker K7 sweeps bit for bit
for every walker-group size (near-tie decisions included), batched energies equal the single-lattice call, whole runs with swaps
equal the NumPy twin (tests/helpers/tempering_twin.py) fed the device energies, swap=False reproduces temperature_scan, split runs
equal one run, equilibrium against exact enumeration, and C-ABI errors."""
import importlib.util
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("tempering_twin", os.path.join(HERE, "helpers", "tempering_twin.py"))
twin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(twin)
dtwin = twin.disorder_twin

TS = [0.4, 0.9, 1.5, 2.27, 5.0]


@pytest.fixture(scope="module")
def hip():
    from tsu import _hip
    return _hip


def _disorder(rows, cols, periodic, seed, field=True):
    rng = np.random.default_rng(seed)
    jr, jd = rng.normal(size=(rows, cols)).astype(np.float32), rng.normal(size=(rows, cols)).astype(np.float32)
    if not periodic:
        jr[:, -1] = 0.0
        jd[-1, :] = 0.0
    return jr, jd, (rng.normal(size=(rows, cols)).astype(np.float32) if field else None)


def _ladders(hip, rows, cols, periodic, Ts, ladders, dis, seed, initial=0):
    pt = hip.TemperingLattice(rows, cols, periodic, len(Ts), ladders)
    pt.set_disorder(*dis)
    pt.set_temperatures(Ts)
    pt.init(seed, initial)
    return pt


def _walkers(hip, rows, cols, periodic, Ts, ladders, dis, seed, initial=0):
    lats = []
    for k in range(ladders):
        for w in range(len(Ts)):
            lat = hip.Lattice(rows, cols, periodic)
            if initial == 0:
                lat.randomize(seed + k * len(Ts) + w)
            else:
                lat.fill(initial)
            lat.set_disorder(*dis)
            lats.append(lat)
    return lats


SHAPES = [(6, 10, True), (37, 53, False), (1, 9, False), (9, 1, False), (128, 1000, True), (1024, 1024, True)]


@pytest.mark.parametrize("rows,cols,periodic", SHAPES)
@pytest.mark.parametrize("group", ["1", "3", "R"])
def test_sweep_and_energy_parity(hip, monkeypatch, rows, cols, periodic, group):
    ladders = 2 if rows * cols < 10 ** 5 else 1
    R = len(TS)
    monkeypatch.setenv("TSU_PT_GROUP", str(R * ladders) if group == "R" else group)
    dis = _disorder(rows, cols, periodic, rows * 31 + cols)
    seed = 1000 + rows
    pt = _ladders(hip, rows, cols, periodic, TS, ladders, dis, seed)
    lats = _walkers(hip, rows, cols, periodic, TS, ladders, dis, seed)
    try:
        for sweep0, n in ((0, 2), (2, 3)):
            pt.run(1, n, swap=False, record=False)
            for g, lat in enumerate(lats):
                lat.disorder_sweep(TS[g % R], n, seed + g, sweep0, 0)
        assert pt.launch_count() == 2 * 5
        E, M = pt.energies()
        for g, lat in enumerate(lats):
            k, w = divmod(g, R)
            got, want = pt.get_spins(k, w), lat.get_spins()
            assert (got == want).all(), f"walker {g}: {int((got != want).sum())} sites differ"
            assert E[k, w] == lat.disorder_energy()  # bit for bit
            assert M[k, w] == lat.observables()[0]
    finally:
        pt.close()
        for lat in lats:
            lat.close()


@pytest.mark.parametrize("rows,cols,periodic", [(64, 64, True), (37, 53, False)])
@pytest.mark.parametrize("group", ["1", "3", "R"])
def test_near_ties_of_walker_zero(hip, monkeypatch, rows, cols, periodic, group):
    """h = the near-tie field of walker 0's key and temperature (J = 0): its decisions of sweep 0 go through the float64 branch."""
    R = len(TS)
    monkeypatch.setenv("TSU_PT_GROUP", str(R) if group == "R" else group)
    seed = 13
    z = np.zeros((rows, cols), np.float32)
    h = dtwin.tie_field(rows, cols, TS[0], seed)
    pt = _ladders(hip, rows, cols, periodic, TS, 1, (z, z, h), seed, initial=1)
    lats = _walkers(hip, rows, cols, periodic, TS, 1, (z, z, h), seed, initial=1)
    try:
        stats = {}
        want0 = dtwin.sweep(np.ones((rows, cols), np.int8), periodic, z, z, h, TS[0], 1, seed, 0, 0, stats=stats)
        assert stats["near"] > 0.9 * stats["sites"], stats
        pt.run(1, 1, swap=False, record=False)
        assert (pt.get_spins(0, 0) == want0).all()
        for w, lat in enumerate(lats):
            lat.disorder_sweep(TS[w], 1, seed + w, 0, 0)
            assert (pt.get_spins(0, w) == lat.get_spins()).all(), w
    finally:
        pt.close()
        for lat in lats:
            lat.close()


@pytest.mark.parametrize("rows,cols,periodic,ladders,Ts", [
    (6, 10, True, 1, [0.4, 0.8, 1.3, 2.0]),
    (37, 53, False, 2, [0.5, 0.7, 1.0, 1.4, 2.0]),
    (1, 9, False, 2, [0.3, 1.0, 3.0]),
    (16, 16, True, 2, list(np.linspace(0.3, 2.0, 8))),
])
def test_run_parity_with_twin(hip, rows, cols, periodic, ladders, Ts):
    dis = _disorder(rows, cols, periodic, 7 + rows)
    seed = 77
    pt = _ladders(hip, rows, cols, periodic, Ts, ladders, dis, seed)
    try:
        R = len(Ts)
        start = [[pt.get_spins(k, w) for w in range(R)] for k in range(ladders)]
        tw = twin.Ladders(start, periodic, dis, Ts, seed)
        for n_rounds, interval in ((4, 2), (3, 1)):
            pt.run(n_rounds, interval, swap=True, record=True)
            hist = pt.history()

            def energies(j, k):
                E = np.empty(R)
                E[hist["walker"][j, k]] = hist["E"][j, k]
                return E
            want = tw.run(n_rounds, interval, True, True, energies)
            assert (hist["walker"] == want["walker"]).all()
            assert (hist["M"] == want["M"]).all()
            if ladders == 2:
                assert (hist["q"] == want["q"]).all()
            st = pt.stats()
            assert (st["attempts"] == tw.attempts).all() and (st["accepts"] == tw.accepts).all()
            assert (st["round_trips"] == tw.trips).all() and (st["walker_at_slot"] == tw.walker_at_slot).all()
            assert st["sweep_count"] == tw.sweeps and st["round_count"] == tw.rounds
        E, _ = pt.energies()
        for k in range(ladders):
            for i in range(R):
                w = tw.walker_at_slot[k, i]
                assert (pt.get_spins(k, i) == tw.spins[k][w]).all()
                assert E[k, w] == pytest.approx(dtwin.energy(tw.spins[k][w], periodic, *dis), rel=1e-12, abs=1e-9)
        assert tw.accepts.sum() > 0
    finally:
        pt.close()


@pytest.mark.parametrize("rows,cols,periodic", [(16, 16, True), (9, 12, False)])
@pytest.mark.parametrize("replicas", [1, 2])
@pytest.mark.parametrize("initial", ["up", "random"])
def test_without_swaps_equals_temperature_scan(hip, rows, cols, periodic, replicas, initial):
    from tsu.models.ising import temperature_scan, tempering_scan
    jr, jd, h = _disorder(rows, cols, periodic, 3)
    kw = dict(n_equilibrate=20, n_measure=6, measure_every=4, seed=100, initial=initial, periodic=periodic,
              couplings=(jr, jd), field=h, replicas=replicas)
    Ts = [0.8, 1.5, 3.0]
    ref = temperature_scan((rows, cols), Ts, **kw)
    out = tempering_scan((rows, cols), Ts, swap=False, **kw)
    for key in ref:
        assert np.array_equal(out[key], ref[key], equal_nan=True), key
    assert np.isnan(out["swap_acceptance"]).all() and out["round_trips"] == 0


def test_split_runs_equal_one_run(hip):
    from tsu.models.ising import LatticeTempering
    jr, jd, h = _disorder(24, 20, True, 5)
    Ts = np.linspace(0.5, 2.5, 6)
    a = LatticeTempering((24, 20), Ts, couplings=(jr, jd), field=h, seed=9, ladders=2)
    b = LatticeTempering((24, 20), Ts, couplings=(jr, jd), field=h, seed=9, ladders=2)
    try:
        a.run(3, 5)
        ha = a.run(4, 5)
        hb = b.run(7, 5)
        for key in ("E", "M", "walker", "q"):
            assert np.array_equal(ha[key], hb[key][3:]), key
        sa, sb = a._pt.stats(), b._pt.stats()
        for key in sa:
            assert np.array_equal(sa[key], sb[key]), key
        for k in range(2):
            for i in range(len(Ts)):
                assert (a.spins(i, k) == b.spins(i, k)).all()
        assert a.sweep_count == 35 and a.energy(0) == b.energy(0)
    finally:
        a._pt.close()
        b._pt.close()


def _exact(jr, jd, periodic, Ts):
    """<E>/N and <q^2> of two independent replicas by enumerating every state (zero field)."""
    rows, cols = jr.shape
    N = rows * cols
    idx = np.arange(2 ** N, dtype=np.int64)
    S = np.empty((2 ** N, N), np.int8)
    for n in range(N):
        S[:, n] = 1 - 2 * ((idx >> n) & 1)
    E = np.zeros(2 ** N)
    for r in range(rows):
        for c in range(cols):
            n = r * cols + c
            if periodic or c + 1 < cols:
                E -= float(jr[r, c]) * (S[:, n] * S[:, r * cols + (c + 1) % cols])
            if periodic or r + 1 < rows:
                E -= float(jd[r, c]) * (S[:, n] * S[:, ((r + 1) % rows) * cols + c])
    out = []
    for T in Ts:
        w = np.exp(-(E - E.min()) / T)
        w /= w.sum()
        C = np.zeros((N, N))
        for lo in range(0, 2 ** N, 1 << 16):
            Sb = S[lo:lo + (1 << 16)].astype(np.float64)
            C += Sb.T @ (Sb * w[lo:lo + (1 << 16), None])
        out.append((float(w @ E) / N, float((C ** 2).sum()) / N ** 2))
    return out


@pytest.mark.parametrize("rows,cols,periodic", [(4, 4, True), (4, 5, False)])
def test_equilibrium_against_exact_enumeration(hip, rows, cols, periodic):
    from tsu.models.ising import LatticeTempering
    jr, jd, _ = _disorder(rows, cols, periodic, 21, field=False)
    Ts = np.linspace(0.3, 2.0, 8)
    N = rows * cols
    pt = LatticeTempering((rows, cols), Ts, couplings=(jr, jd), periodic=periodic, seed=5, ladders=2)
    try:
        pt.run(400, 5, record=False)
        h = pt.run(8000, 5)
        nb = 20
        exact = _exact(jr, jd, periodic, Ts)
        for i, (e_ex, q2_ex) in enumerate(exact):
            e_b = (h["E"][:, i] / N).reshape(nb, -1).mean(axis=1)
            q_b = ((h["q"][:, i] / N) ** 2).reshape(nb, -1).mean(axis=1)
            for b, ex in ((e_b, e_ex), (q_b, q2_ex)):
                se = b.std(ddof=1) / math.sqrt(nb)
                assert abs(b.mean() - ex) < 4 * se + 1e-4, (i, Ts[i], b.mean(), ex, se)
        assert (pt.acceptance > 0).all(), pt.acceptance
        assert pt.round_trips >= 1
    finally:
        pt._pt.close()


def test_errors(hip):
    z = np.zeros((8, 8), np.float32)
    with pytest.raises(ValueError):
        hip.TemperingLattice(8, 8, True, 257, 1)
    with pytest.raises(ValueError):
        hip.TemperingLattice(8, 8, True, 1, 1)
    with pytest.raises(ValueError):
        hip.TemperingLattice(8, 8, True, 4, 3)
    with pytest.raises(hip.UnsupportedError):  # a periodic lattice K7 does not take
        hip.TemperingLattice(5, 8, True, 4, 1)
    pt = hip.TemperingLattice(8, 8, True, 4, 2)
    try:
        with pytest.raises(ValueError, match="set_disorder"):
            pt.run(1, 1)
        with pytest.raises(ValueError, match="positive"):
            pt.set_temperatures([1.0, 0.0, 2.0, 3.0])
        with pytest.raises(ValueError, match="positive"):
            pt.set_temperatures([1.0, np.nan, 2.0, 3.0])
        with pytest.raises(ValueError, match="non-finite"):
            pt.set_disorder(np.full((8, 8), np.inf, np.float32), z)
        pt.set_disorder(z, z)
        with pytest.raises(ValueError, match="set_temperatures"):
            pt.run(1, 1)
        pt.set_temperatures([0.5, 1.0, 2.0, 3.0])
        with pytest.raises(ValueError, match="init"):
            pt.run(1, 1)
        pt.init(3)
        with pytest.raises(ValueError):
            pt.run(1, 0)
        with pytest.raises(ValueError, match="out of range"):
            pt.get_spins(0, 4)
        with pytest.raises(ValueError, match="out of range"):
            pt.get_spins(2, 0)
        with pytest.raises(ValueError, match="out of range"):
            pt.set_spins(-1, 0, np.ones((8, 8), np.int8))
        pt.run(2, 1)
        assert pt.history()["q"].shape == (2, 4)
    finally:
        pt.close()
    opn = hip.TemperingLattice(5, 7, False, 3, 1)
    try:
        with pytest.raises(ValueError, match="last column"):
            opn.set_disorder(np.ones((5, 7), np.float32), np.zeros((5, 7), np.float32))
    finally:
        opn.close()

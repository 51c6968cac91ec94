"""K8 parallel tempering on the GPU (tsu_pt3d_*, csrc/ising3d.hip): batched sweeps equal the NumPy twin of K8 bit for bit for every
walker-group size (near-tie decisions included), batched energies equal the single-lattice call bit for bit, whole runs with swaps
equal the twin (tests/helpers/tempering3d_twin.py) fed the device energies, swap=False reproduces temperature_scan_3d, a one-layer
ladder equals the 2-D ladder, split runs equal one run, equilibrium against exact enumeration, and C-ABI errors."""
import importlib.util
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("tempering3d_twin", os.path.join(HERE, "helpers", "tempering3d_twin.py"))
twin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(twin)
ltwin = twin.lattice3d_twin

TS = [0.4, 0.9, 1.5, 2.27, 5.0]


@pytest.fixture(scope="module")
def hip():
    from tsu import _hip
    return _hip


def _disorder(shape, periodic, seed, field=True):
    rng = np.random.default_rng(seed)
    jr, jd, jl = (rng.normal(size=shape).astype(np.float32) for _ in range(3))
    pz, pr, pc = ltwin.axes(periodic)
    if not pc:
        jr[:, :, -1] = 0.0
    if not pr:
        jd[:, -1, :] = 0.0
    if not pz:
        jl[-1, :, :] = 0.0
    return jr, jd, jl, (rng.normal(size=shape).astype(np.float32) if field else None)


def _ladders(hip, shape, periodic, Ts, ladders, dis, seed, initial=0):
    pt = hip.TemperingLattice3D(*shape, periodic, len(Ts), ladders)
    pt.set_disorder(*dis)
    pt.set_temperatures(Ts)
    pt.init(seed, initial)
    return pt


def _same(got, want, what):
    assert (got == want).all(), f"{what}: {int((got != want).sum())} of {want.size} sites differ"


SHAPES = [((64, 64, 64), True), ((3, 5, 37), False), ((8, 6, 40), (True, False, True)), ((4, 6, 1040), (False, True, True))]


@pytest.mark.parametrize("shape,periodic", SHAPES)
@pytest.mark.parametrize("ladders", [1, 2])
@pytest.mark.parametrize("group", ["1", "3", "R"])
def test_sweep_and_energy_parity(hip, monkeypatch, shape, periodic, ladders, group):
    """After n sweeps without swaps every walker's spins equal lattice3d_twin's; every E equals tsu_ising3d_energy of a single
    Lattice3D holding the same spins and disorder bit for bit, and the sum of spins equals tsu_ising3d_sum_spins."""
    R = len(TS)
    monkeypatch.setenv("TSU_PT_GROUP", str(R * ladders) if group == "R" else group)
    dis = _disorder(shape, periodic, shape[0] * 31 + shape[2])
    seed = 1000 + shape[1]
    pt = _ladders(hip, shape, periodic, TS, ladders, dis, seed)
    one = hip.Lattice3D(*shape, periodic)
    try:
        one.set_disorder(*dis)
        start = [[pt.get_spins(k, w) for w in range(R)] for k in range(ladders)]
        want0 = twin.initial_spins(shape, seed, ladders * R)
        for sweep0, n in ((0, 1), (1, 2)):
            pt.run(1, n, swap=False, record=False)
        assert pt.launch_count() == 2 * 3
        E, M = pt.energies()
        for k in range(ladders):
            for w in range(R):
                g = k * R + w
                _same(start[k][w], want0[g], f"initial draw of walker {g}")
                got = pt.get_spins(k, w)
                _same(got, ltwin.sweep(start[k][w], periodic, *dis, TS[w], 3, seed + g, 0, 0), f"walker {g} {shape} group {group}")
                one.set_spins(got)
                assert E[k, w] == one.energy(), (g, E[k, w], one.energy())  # bit for bit
                assert M[k, w] == one.sum_spins()
    finally:
        pt.close()
        one.close()


@pytest.mark.parametrize("shape,periodic", [((64, 64, 64), True), ((3, 5, 37), False), ((8, 6, 40), (True, False, True))])
@pytest.mark.parametrize("group", ["1", "3", "R"])
@pytest.mark.parametrize("variant", ["J0", "gauss"])
def test_near_ties_of_walker_zero(hip, monkeypatch, shape, periodic, group, variant):
    """h = lattice3d_twin.tie_field of walker 0's key and temperature, with J = 0 and with Gaussian J (the tie field computed for
    walker 0's actual start state): every decision of its sweep 0 lies within 2^-16 of its threshold, so it goes through the float64
    branch inside the walker loop, and the spins still equal the twin's."""
    R = len(TS)
    monkeypatch.setenv("TSU_PT_GROUP", str(R) if group == "R" else group)
    seed = 13
    start = twin.initial_spins(shape, seed, R)
    if variant == "J0":
        jr = jd = jl = np.zeros(shape, np.float32)
        h = ltwin.tie_field(shape, TS[0], seed)
    else:
        jr, jd, jl, _ = _disorder(shape, periodic, 31, field=False)
        h = ltwin.tie_field(shape, TS[0], seed, 0, spins=start[0], periodic=periodic, couplings=(jr, jd, jl))
    pt = _ladders(hip, shape, periodic, TS, 1, (jr, jd, jl, h), seed)
    try:
        _same(pt.get_spins(0, 0), start[0], "walker 0's start")
        stats = {}
        want0 = ltwin.sweep(start[0], periodic, jr, jd, jl, h, TS[0], 1, seed, 0, 0, stats=stats)
        assert stats["near"] == stats["sites"], stats
        pt.run(1, 1, swap=False, record=False)
        _same(pt.get_spins(0, 0), want0, f"near ties of walker 0 {shape} {variant} group {group}")
        for w in range(1, R):
            _same(pt.get_spins(0, w), ltwin.sweep(start[w], periodic, jr, jd, jl, h, TS[w], 1, seed + w, 0, 0), f"walker {w}")
    finally:
        pt.close()


@pytest.mark.parametrize("shape,periodic", [((8, 8, 8), True), ((3, 5, 9), False)])
@pytest.mark.parametrize("ladders", [1, 2])
def test_run_parity_with_twin(hip, shape, periodic, ladders):
    Ts = list(np.linspace(0.5, 2.4, 6))
    dis = _disorder(shape, periodic, 7 + shape[0])
    seed = 77
    pt = _ladders(hip, shape, periodic, Ts, ladders, dis, seed)
    try:
        R = len(Ts)
        start = [[pt.get_spins(k, w) for w in range(R)] for k in range(ladders)]
        tw = twin.Ladders(start, periodic, dis, Ts, seed)
        for n_rounds, interval in ((20, 2), (12, 1)):
            pt.run(n_rounds, interval, swap=True, record=True)
            hist = pt.history()

            def energies(j, k):
                E = np.empty(R)
                E[hist["walker"][j, k]] = hist["E"][j, k]
                return E
            want = tw.run(n_rounds, interval, True, True, energies)
            assert (hist["walker"] == want["walker"]).all()
            assert (hist["E"] == want["E"]).all()
            assert (hist["M"] == want["M"]).all()
            if ladders == 2:
                assert (hist["q"] == want["q"]).all()
            else:
                assert hist["q"] is None
            st = pt.stats()
            assert (st["attempts"] == tw.attempts).all() and (st["accepts"] == tw.accepts).all()
            assert (st["round_trips"] == tw.trips).all() and (st["walker_at_slot"] == tw.walker_at_slot).all()
            assert st["sweep_count"] == tw.sweeps and st["round_count"] == tw.rounds
        E, _ = pt.energies()
        for k in range(ladders):
            for i in range(R):
                w = tw.walker_at_slot[k, i]
                _same(pt.get_spins(k, i), tw.spins[k][w], f"ladder {k} slot {i}")
                assert E[k, w] == pytest.approx(ltwin.energy(tw.spins[k][w], periodic, *dis), rel=1e-12, abs=1e-9)
        assert tw.accepts.sum() > 0 and tw.rounds == 32
    finally:
        pt.close()


@pytest.mark.parametrize("shape,periodic", [((4, 6, 8), True), ((3, 5, 9), False)])
@pytest.mark.parametrize("replicas", [1, 2])
@pytest.mark.parametrize("initial", ["up", "random"])
def test_without_swaps_equals_temperature_scan_3d(hip, shape, periodic, replicas, initial):
    from tsu.models.ising import temperature_scan_3d, tempering_scan_3d
    jr, jd, jl, h = _disorder(shape, periodic, 3)
    kw = dict(n_equilibrate=20, n_measure=6, measure_every=4, seed=100, initial=initial, periodic=periodic,
              couplings=(jr, jd, jl), field=h, replicas=replicas)
    Ts = [0.8, 1.5, 3.0]
    ref = temperature_scan_3d(shape, Ts, **kw)
    out = tempering_scan_3d(shape, Ts, swap=False, **kw)
    for key in ref:
        assert np.array_equal(out[key], ref[key], equal_nan=True), key
    assert set(out) == set(ref) | {"swap_acceptance", "round_trips"}
    assert np.isnan(out["swap_acceptance"]).all() and out["round_trips"] == 0


@pytest.mark.parametrize("rows,cols,periodic", [(6, 40, True), (5, 37, False)])
def test_one_layer_ladder_has_the_2d_ladders_spins(hip, rows, cols, periodic):
    """D = 1, open z, swap=False: the spins of the 2-D TemperingLattice on the same arrays.  Then four swapping, recorded rounds
    on both: with one open layer energy_lane<3> adds h, J_right and J_down in energy_lane<2>'s order over the same lanes, so the
    energies, and with them the swaps, the history, the counters and the spins at every slot, are equal exactly."""
    shape = (1, rows, cols)
    jr, jd, _, h = _disorder(shape, (False, periodic, periodic), 11)
    seed = 21
    p3 = _ladders(hip, shape, (False, periodic, periodic), TS, 2, (jr, jd, np.zeros(shape, np.float32), h), seed)
    p2 = hip.TemperingLattice(rows, cols, periodic, len(TS), 2)
    try:
        p2.set_disorder(jr.reshape(rows, cols), jd.reshape(rows, cols), h.reshape(rows, cols))
        p2.set_temperatures(TS)
        p2.init(seed, 0)
        for n in (2, 3):
            p3.run(1, n, swap=False, record=False)
            p2.run(1, n, swap=False, record=False)
        for k in range(2):
            for w in range(len(TS)):
                _same(p3.get_spins(k, w).reshape(rows, cols), p2.get_spins(k, w), f"ladder {k} walker {w}")
        p3.run(4, 3, swap=True, record=True)
        p2.run(4, 3, swap=True, record=True)
        h3, h2 = p3.history(), p2.history()
        for key in ("E", "M", "walker", "q"):
            assert np.array_equal(h3[key], h2[key]), key
        s3, s2 = p3.stats(), p2.stats()
        assert set(s3) == set(s2)
        for key in s3:
            assert np.array_equal(s3[key], s2[key]), key
        for a3, a2 in zip(p3.energies(), p2.energies()):
            assert np.array_equal(a3, a2)
        for k in range(2):
            for slot in range(len(TS)):
                _same(p3.get_spins(k, slot).reshape(rows, cols), p2.get_spins(k, slot), f"ladder {k} slot {slot}")
    finally:
        p3.close()
        p2.close()


def test_split_runs_equal_one_run(hip):
    from tsu.models.ising import LatticeTempering3D
    shape = (6, 4, 20)
    jr, jd, jl, h = _disorder(shape, True, 5)
    Ts = np.linspace(0.5, 2.5, 6)
    a = LatticeTempering3D(shape, Ts, couplings=(jr, jd, jl), field=h, seed=9, ladders=2)
    b = LatticeTempering3D(shape, Ts, couplings=(jr, jd, jl), field=h, seed=9, ladders=2)
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
        assert a.spins(0).shape == shape and (a.walker_at_slot == b.walker_at_slot).all()
    finally:
        a._pt.close()
        b._pt.close()


@pytest.mark.parametrize("R", [2, 5, 33])
@pytest.mark.parametrize("ladders", [1, 2])
def test_launch_count_does_not_depend_on_the_ladder(hip, monkeypatch, R, ladders):
    """One launch per half-sweep for all walkers of both ladders: 2 swap_interval launches per round whatever R is."""
    monkeypatch.delenv("TSU_PT_GROUP", raising=False)
    shape = (4, 4, 8)
    pt = _ladders(hip, shape, True, np.linspace(0.5, 3.0, R), ladders, _disorder(shape, True, 1), 4)
    try:
        pt.run(3, 7)
        assert pt.launch_count() == 3 * 2 * 7
        pt.run(2, 1, swap=False, record=False)
        assert pt.launch_count() == 3 * 2 * 7 + 2 * 2
    finally:
        pt.close()


# ---------------------------------------------------------------- equilibrium against exact enumeration
ENUM_TS = np.linspace(0.3, 2.0, 8)
# (shape, periodic, disorder seed, ladder seed): picked by the rehearsal described in the test's docstring
ENUM_CASES = [((2, 3, 2), False, 21, 5), ((4, 2, 2), (True, False, False), 21, 5)]


def exact_enumeration(shape, periodic, jr, jd, jl, Ts):
    """<E>/N and <q^2> of two independent replicas by enumerating every state (zero field)."""
    D, R, C = shape
    pz, pr, pc = ltwin.axes(periodic)
    N = D * R * C
    idx = np.arange(2 ** N, dtype=np.int64)
    S = np.empty((2 ** N, N), np.int8)
    for n in range(N):
        S[:, n] = 1 - 2 * ((idx >> n) & 1)
    site = lambda z, r, c: (z * R + r) * C + c  # noqa: E731
    E = np.zeros(2 ** N)
    for z in range(D):
        for r in range(R):
            for c in range(C):
                n = site(z, r, c)
                if pc or c + 1 < C:
                    E -= float(jr[z, r, c]) * (S[:, n] * S[:, site(z, r, (c + 1) % C)])
                if pr or r + 1 < R:
                    E -= float(jd[z, r, c]) * (S[:, n] * S[:, site(z, (r + 1) % R, c)])
                if pz or z + 1 < D:
                    E -= float(jl[z, r, c]) * (S[:, n] * S[:, site((z + 1) % D, r, c)])
    out = []
    for T in Ts:
        w = np.exp(-(E - E.min()) / T)
        w /= w.sum()
        Cm = np.zeros((N, N))
        for lo in range(0, 2 ** N, 1 << 16):
            Sb = S[lo:lo + (1 << 16)].astype(np.float64)
            Cm += Sb.T @ (Sb * w[lo:lo + (1 << 16), None])
        out.append((float(w @ E) / N, float((Cm ** 2).sum()) / N ** 2))
    return out


def batch_deviations(E, q, N, exact, nb=20):
    """Per temperature and observable (E/N, q^2): (mean of the nb batch means, exact value, standard error of the mean)."""
    rows = []
    for i, (e_ex, q2_ex) in enumerate(exact):
        e_b = (E[:, i] / N).reshape(nb, -1).mean(axis=1)
        q_b = ((q[:, i] / N) ** 2).reshape(nb, -1).mean(axis=1)
        for b, ex in ((e_b, e_ex), (q_b, q2_ex)):
            rows.append((i, float(b.mean()), ex, float(b.std(ddof=1) / math.sqrt(nb))))
    return rows


@pytest.mark.parametrize("shape,periodic,dseed,seed", ENUM_CASES)
def test_equilibrium_against_exact_enumeration(hip, shape, periodic, dseed, seed):
    """Two ladders over 8 temperatures, Gaussian J, zero field: 400 discarded rounds, 8000 recorded rounds of 5 sweeps, 20 batch
    means; <E>/N and <q^2> at every temperature within 4 standard errors + 1e-4 of the exact enumeration (the rule and lengths of
    the 2-D test), every pair's acceptance > 0 and at least one round trip.

    The disorder and ladder seeds were picked by rehearsing this very ladder with the NumPy twin on its own float64 energies (it
    checks the statistics, not the bits).  Two (disorder seed, ladder seed) pairs were rehearsed per lattice, (21, 5) and (22, 6);
    all four rehearsals met the rule and the first pair was kept.  Worst deviation of the kept rehearsals over the 16 figures, in
    units of the standard error: 2.45 (open 2x3x2) and 2.20 (z-periodic 4x2x2); every pair's acceptance lay in 0.59 ... 0.88,
    4495 and 3085 round trips.  A device run that disagrees is a finding, not a reason to pick other seeds.  (The first device
    run gave the rehearsals' figures digit for digit: the device's energies led to the twin's swap decisions throughout.)
    """
    from tsu.models.ising import LatticeTempering3D
    jr, jd, jl, _ = _disorder(shape, periodic, dseed, field=False)
    N = int(np.prod(shape))
    pt = LatticeTempering3D(shape, ENUM_TS, couplings=(jr, jd, jl), periodic=periodic, seed=seed, ladders=2)
    try:
        pt.run(400, 5, record=False)
        h = pt.run(8000, 5)
        exact = exact_enumeration(shape, periodic, jr, jd, jl, ENUM_TS)
        worst = 0.0
        for i, mean, ex, se in batch_deviations(h["E"], h["q"], N, exact):
            print(f"T={ENUM_TS[i]:.3f} mean={mean:.6f} exact={ex:.6f} se={se:.2e} dev={(mean - ex) / se if se else 0.0:+.2f} se")
            worst = max(worst, abs(mean - ex) / se if se else 0.0)
            assert abs(mean - ex) < 4 * se + 1e-4, (i, ENUM_TS[i], mean, ex, se)
        print(f"worst deviation {worst:.2f} se; acceptance {pt.acceptance}; round trips {pt.round_trips}")
        assert (pt.acceptance > 0).all(), pt.acceptance
        assert pt.round_trips >= 1
    finally:
        pt._pt.close()


def test_errors(hip):
    S = (4, 4, 8)
    z = np.zeros(S, np.float32)
    with pytest.raises(ValueError):
        hip.TemperingLattice3D(*S, True, 257, 1)
    with pytest.raises(ValueError):
        hip.TemperingLattice3D(*S, True, 1, 1)
    with pytest.raises(ValueError):
        hip.TemperingLattice3D(*S, True, 4, 3)
    with pytest.raises(ValueError, match="positive"):
        hip.TemperingLattice3D(4, 0, 8, False, 4, 1)
    with pytest.raises(hip.UnsupportedError, match="even length"):  # a periodic axis K8 does not take
        hip.TemperingLattice3D(5, 4, 8, True, 4, 1)
    pt = hip.TemperingLattice3D(*S, True, 4, 2)
    try:
        with pytest.raises(ValueError, match="set_disorder"):
            pt.run(1, 1)
        with pytest.raises(ValueError, match="positive"):
            pt.set_temperatures([1.0, 0.0, 2.0, 3.0])
        with pytest.raises(ValueError, match="positive"):
            pt.set_temperatures([1.0, np.nan, 2.0, 3.0])
        with pytest.raises(ValueError):
            pt.set_temperatures([1.0, 2.0, 3.0])
        with pytest.raises(ValueError, match="non-finite"):
            pt.set_disorder(np.full(S, np.inf, np.float32), z, z)
        pt.set_disorder(z, z, z)
        with pytest.raises(ValueError, match="set_temperatures"):
            pt.run(1, 1)
        pt.set_temperatures([0.5, 1.0, 2.0, 3.0])
        with pytest.raises(ValueError, match="init"):
            pt.run(1, 1)
        with pytest.raises(ValueError, match="initial"):
            pt.init(3, 2)
        pt.init(3)
        with pytest.raises(ValueError):
            pt.run(1, 0)
        with pytest.raises(ValueError, match="out of range"):
            pt.get_spins(0, 4)
        with pytest.raises(ValueError, match="out of range"):
            pt.get_spins(2, 0)
        with pytest.raises(ValueError, match="out of range"):
            pt.set_spins(-1, 0, np.ones(S, np.int8))
        with pytest.raises(ValueError):
            pt.set_spins(0, 0, np.ones((4, 4, 7), np.int8))  # a wrong shape
        up = np.ones(S, np.int8)
        pt.set_spins(1, 2, up)
        assert (pt.get_spins(1, 2) == up).all()
        pt.run(2, 1)
        assert pt.history()["q"].shape == (2, 4)
    finally:
        pt.close()
    opn = hip.TemperingLattice3D(3, 5, 7, False, 3, 1)
    try:
        with pytest.raises(ValueError, match="last column"):
            opn.set_disorder(np.ones((3, 5, 7), np.float32), np.zeros((3, 5, 7), np.float32), np.zeros((3, 5, 7), np.float32))
        with pytest.raises(ValueError, match="last layer"):
            opn.set_disorder(np.zeros((3, 5, 7), np.float32), np.zeros((3, 5, 7), np.float32), np.ones((3, 5, 7), np.float32))
    finally:
        opn.close()

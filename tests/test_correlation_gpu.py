"""Correlation length on the GPU (csrc/corr_dev.h): axis profiles of single lattices, pairs and ladder slots equal the NumPy twin
(tests/helpers/correlation_twin.py) exactly, fourier_modes and the modes a ladder records equal the twin's bit for bit, switching the
recording on changes nothing else, and <|F|^2> of small glasses agrees with full enumeration."""
import importlib.util
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("correlation_twin", os.path.join(HERE, "helpers", "correlation_twin.py"))
twin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(twin)

TS = [0.4, 0.9, 1.5, 2.27, 5.0]


@pytest.fixture(scope="module")
def hip():
    from tsu import _hip
    return _hip


def _random(shape, seed):
    return np.where(np.random.default_rng(seed).integers(0, 2, size=shape) == 1, 1, -1).astype(np.int8)


def _stripes(shape, axis):
    """+1 / -1 alternating along `axis` in runs of one (axis length odd: one more +1 slice)."""
    idx = np.indices(shape)[axis]
    return np.where(idx % 2 == 0, 1, -1).astype(np.int8)


def _configs(shape):
    """(name, a, b or None): random spins and stripes along each axis, single and as pairs."""
    out = [("random", _random(shape, 11), None), ("random pair", _random(shape, 12), _random(shape, 13))]
    for d in range(len(shape)):
        st = _stripes(shape, d)
        out.append((f"stripes {d}", st, None))
        out.append((f"stripes {d} x random", st, _random(shape, 14 + d)))
        out.append((f"stripes {d} x stripes {(d + 1) % len(shape)}", st, _stripes(shape, (d + 1) % len(shape))))
    return out


def _equal_profiles(got, want, what):
    assert len(got) == len(want)
    for d, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.int64
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: axis {d}")


CASES_2D = [((6, 10), True), ((33, 50), False), ((130, 272), True), ((4, 16400), True)]
CASES_3D = [((3, 5, 18), False), ((4, 6, 34), True), ((16, 16, 16), True), ((2, 130, 20), (False, True, True)), ((1, 8, 20), False)]


@pytest.mark.parametrize("shape,periodic", CASES_2D)
def test_profiles_2d(hip, shape, periodic):
    """Exact int64 profiles, single and pair; every profile sums to what observables / overlap return.  4 x 16400 is wider than one
    column tile of 4096."""
    A, B = hip.Lattice(*shape, periodic), hip.Lattice(*shape, periodic)
    try:
        for name, a, b in _configs(shape):
            A.set_spins(a)
            if b is not None:
                B.set_spins(b)
            got = A.profiles(None if b is None else B)
            _equal_profiles(got, twin.profiles(a, b), f"{shape} {name}")
            total = A.observables()[0] if b is None else A.overlap(B)
            assert all(int(P.sum()) == total for P in got), (name, total)
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("shape,periodic", CASES_3D)
def test_profiles_3d(hip, shape, periodic):
    A, B = hip.Lattice3D(*shape, periodic), hip.Lattice3D(*shape, periodic)
    try:
        for name, a, b in _configs(shape):
            A.set_spins(a)
            if b is not None:
                B.set_spins(b)
            got = A.profiles(None if b is None else B)
            _equal_profiles(got, twin.profiles(a, b), f"{shape} {name}")
            total = A.sum_spins() if b is None else A.overlap(B)
            assert all(int(P.sum()) == total for P in got), (name, total)
    finally:
        A.close()
        B.close()


def test_one_layer_profiles_equal_the_2d_ones(hip):
    a, b = _random((8, 20), 21), _random((8, 20), 22)
    L2a, L2b = hip.Lattice(8, 20, False), hip.Lattice(8, 20, False)
    L3a, L3b = hip.Lattice3D(1, 8, 20, False), hip.Lattice3D(1, 8, 20, False)
    try:
        L2a.set_spins(a), L2b.set_spins(b), L3a.set_spins(a), L3b.set_spins(b)
        for other2, other3 in ((None, None), (L2b, L3b)):
            p2, p3 = L2a.profiles(other2), L3a.profiles(other3)
            np.testing.assert_array_equal(p3[1], p2[0])
            np.testing.assert_array_equal(p3[2], p2[1])
            assert p3[0].shape == (1,) and p3[0][0] == p2[0].sum()
    finally:
        for lat in (L2a, L2b, L3a, L3b):
            lat.close()


def _half(shape, axis):
    idx = np.indices(shape)[axis]
    return np.where(idx < shape[axis] // 2, 1, -1).astype(np.int8)


def _same_modes(got, want, what):
    """Bit for bit, NaN on the same (open) axes."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.complex128, what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(got[ok].view(np.float64).view(np.uint64), want[ok].view(np.float64).view(np.uint64), err_msg=what)


@pytest.mark.parametrize("shape,periodic", [((6, 10), True), ((33, 50), False), ((130, 272), True), ((4, 16400), True),
                                            ((4, 6, 34), True), ((2, 130, 20), (False, True, True)), ((16, 16, 16), True)])
def test_fourier_modes(hip, shape, periodic):
    """fourier_modes equals the twin bit for bit (NaN on open axes), single and pair; a half-up / half-down configuration along a
    periodic axis of length L gives 4 (N / L) / (1 - exp(2 pi i / L)) within 1e-9 N (the bound of the CPU test)."""
    from tsu.models.ising import IsingModel2D, IsingModel3D
    cls = IsingModel2D if len(shape) == 2 else IsingModel3D
    per = twin.lattice3d_twin.axes(periodic) if len(shape) == 3 else (bool(periodic),) * 2
    N = int(np.prod(shape))
    m, o = cls(shape, periodic=periodic, seed=1), cls(shape, periodic=periodic, seed=2)
    a, b = m.spins, o.spins
    assert (a != b).any()
    _same_modes(m.fourier_modes(), twin.modes(twin.profiles(a), per), f"{shape} single")
    _same_modes(m.fourier_modes(o), twin.modes(twin.profiles(a, b), per), f"{shape} pair")
    _equal_profiles(m.axis_profiles(o), twin.profiles(a, b), f"{shape} axis_profiles")
    for d in range(len(shape)):
        if not per[d]:
            continue
        m.spins = _half(shape, d)
        got = m.fourier_modes()
        L = shape[d]
        want = 4.0 * (N / L) / (1.0 - np.exp(2j * np.pi / L))
        assert abs(got[d] - want) <= 1e-9 * N, (d, got[d], want)
        for e in range(len(shape)):
            if e != d and per[e]:
                assert abs(got[e]) <= 1e-9 * N  # constant along the other axes: no k_min component
        _same_modes(got, twin.modes(twin.profiles(m.spins), per), f"{shape} half {d}")


# ---------------------------------------------------------------- ladders
def _disorder(shape, periodic, seed):
    rng = np.random.default_rng(seed)
    if len(shape) == 2:
        jr, jd, h = (rng.normal(size=shape).astype(np.float32) for _ in range(3))
        if not periodic:
            jr[:, -1] = 0.0
            jd[-1, :] = 0.0
        return (jr, jd), h
    jr, jd, jl, h = (rng.normal(size=shape).astype(np.float32) for _ in range(4))
    pz, pr, pc = twin.lattice3d_twin.axes(periodic)
    if not pc:
        jr[:, :, -1] = 0.0
    if not pr:
        jd[:, -1, :] = 0.0
    if not pz:
        jl[-1, :, :] = 0.0
    return (jr, jd, jl), h


LADDER_CASES = [((12, 20), True), ((4, 6, 18), (True, False, True))]


def _ladder(shape, periodic, ladders, seed=50, correlation=True, **kw):
    from tsu.models.ising import LatticeTempering, LatticeTempering3D
    J, h = _disorder(shape, periodic, 7)
    cls = LatticeTempering if len(shape) == 2 else LatticeTempering3D
    return cls(shape, TS, couplings=J, field=h, periodic=periodic, seed=seed, ladders=ladders, correlation=correlation, **kw)


def _axes(shape, periodic):
    return twin.lattice3d_twin.axes(periodic) if len(shape) == 3 else (bool(periodic),) * 2


def _twin_row(pt, shape, periodic):
    """twin.modes of the walkers now at every slot, and their profiles."""
    rows, profs = [], []
    for slot in range(len(TS)):
        a = pt.spins(slot, 0)
        b = pt.spins(slot, 1) if pt.ladders == 2 else None
        profs.append(twin.profiles(a, b))
        rows.append(twin.modes(profs[-1], _axes(shape, periodic)))
    return np.array(rows), profs


@pytest.mark.parametrize("shape,periodic", LADDER_CASES)
@pytest.mark.parametrize("ladders", [1, 2])
def test_ladder_modes_equal_the_twin(hip, shape, periodic, ladders):
    """Six runs of one recorded round of two sweeps: the row each records equals twin.modes of the spins read back afterwards (the
    walkers the swap pass left at each slot), bit for bit; tsu_pt*_profiles equals the twin's profiles.  Then one run of six rounds
    on a fresh ladder: its last row equals the same, and the first run's row is the row of the six single runs."""
    pt = _ladder(shape, periodic, ladders)
    try:
        first = None
        for k in range(6):
            h = pt.run(1, swap_interval=2)
            assert h["modes"].shape == (1, len(TS), len(shape))
            want, profs = _twin_row(pt, shape, periodic)
            _same_modes(h["modes"][0], want, f"run {k}")
            _same_modes(pt.history()["modes"][0], want, f"run {k} history()")
            for slot in range(len(TS)):
                _equal_profiles(pt.axis_profiles(slot), profs[slot], f"run {k} slot {slot}")
            first = h["modes"][0] if first is None else first
        last = want
    finally:
        pt._pt.close()
    pt = _ladder(shape, periodic, ladders)
    try:
        h = pt.run(6, 2)
        assert h["modes"].shape == (6, len(TS), len(shape))
        want, _ = _twin_row(pt, shape, periodic)
        _same_modes(h["modes"][-1], want, "last row of run(6, 2)")
        _same_modes(h["modes"][-1], last, "six runs of one round against one run of six")
        _same_modes(h["modes"][0], first, "first row")
    finally:
        pt._pt.close()


def _everything(pt):
    st = pt._pt.stats()
    spins = [pt.spins(s, k) for k in range(pt.ladders) for s in range(len(TS))]
    return st, spins


@pytest.mark.parametrize("shape,periodic,kw,ladders", [((12, 20), True, {}, 1), ((12, 20), True, {}, 2),
                                                       ((12, 20), True, {"cluster_moves": 2}, 2),
                                                       ((4, 6, 18), (True, False, True), {}, 1),
                                                       ((4, 6, 18), (True, False, True), {}, 2)])
def test_opt_in_changes_nothing_else(hip, shape, periodic, kw, ladders):
    """The same seed with and without correlation: identical histories, swap statistics, round trips, launch counts, cluster-move
    statistics and final spins; history_modes refuses a run that recorded none."""
    on, off = _ladder(shape, periodic, ladders, **kw), _ladder(shape, periodic, ladders, correlation=False, **kw)
    try:
        on.run(3, 2, record=False)
        off.run(3, 2, record=False)
        h_on, h_off = on.run(8, 3), off.run(8, 3)
        assert "modes" in h_on and "modes" not in h_off
        assert sorted(k for k in h_on if k != "modes") == sorted(h_off)
        raw_on, raw_off = on._pt.history(), off._pt.history()
        for k in ("E", "M", "walker") + (("q",) if ladders == 2 else ()):
            np.testing.assert_array_equal(raw_on[k], raw_off[k], err_msg=k)
        (st_on, s_on), (st_off, s_off) = _everything(on), _everything(off)
        for k in ("attempts", "accepts", "round_trips", "walker_at_slot"):
            np.testing.assert_array_equal(st_on[k], st_off[k], err_msg=k)
        assert st_on["sweep_count"] == st_off["sweep_count"] and st_on["round_count"] == st_off["round_count"]
        for x, y in zip(s_on, s_off):
            np.testing.assert_array_equal(x, y)
        assert on._pt.launch_count() == off._pt.launch_count()
        if kw:
            for k, v in on.cluster_stats.items():
                np.testing.assert_array_equal(v, off.cluster_stats[k], err_msg=k)
        with pytest.raises(ValueError, match="recorded no modes"):
            off._pt.history_modes()
        on.run(2, 1, record=False)
        with pytest.raises(ValueError, match="recorded no modes"):
            on._pt.history_modes()
    finally:
        on._pt.close()
        off._pt.close()


SCAN_KEYS = {"magnetization", "energy", "susceptibility", "specific_heat", "temperatures", "swap_acceptance", "round_trips"}


def test_scans_keep_their_keys_and_gain_the_correlation_ones(hip):
    from tsu.models.ising import tempering_scan, tempering_scan_3d, temperature_scan
    J, h = _disorder((12, 20), True, 7)
    kw = dict(couplings=J, field=h, n_equilibrate=20, n_measure=12, measure_every=2, seed=3, initial="random")
    base = tempering_scan((12, 20), TS, **kw)
    assert set(base) == SCAN_KEYS
    off = tempering_scan((12, 20), TS, correlation=False, **kw)
    on = tempering_scan((12, 20), TS, correlation=True, **kw)
    assert set(off) == SCAN_KEYS and set(on) == SCAN_KEYS | {"chi_k", "xi", "xi_over_L"}
    for k in SCAN_KEYS:
        np.testing.assert_array_equal(np.asarray(on[k]), np.asarray(base[k]), err_msg=k)
        np.testing.assert_array_equal(np.asarray(off[k]), np.asarray(base[k]), err_msg=k)
    assert on["chi_k"].shape == on["xi"].shape == (len(TS), 2) and on["xi_over_L"].shape == (len(TS),)
    assert (on["chi_k"] > 0).all()
    two = tempering_scan((12, 20), TS, replicas=2, correlation=True, **kw)
    assert set(two) == SCAN_KEYS | {"overlap", "overlap_sq", "binder", "chi_k", "xi", "xi_over_L"}
    # without swaps the ladder is the single-lattice scan: the host-summed modes of temperature_scan are the device's
    for replicas in (1, 2):
        a = tempering_scan((12, 20), TS, replicas=replicas, swap=False, correlation=True, **kw)
        b = temperature_scan((12, 20), TS, replicas=replicas, correlation=True, **kw)
        # the same |F|^2 per measurement, averaged over 12 of them along different array axes: a few ulp apart at most
        np.testing.assert_allclose(a["chi_k"], b["chi_k"], rtol=1e-13, err_msg=f"chi_k replicas={replicas}")
    J3, h3 = _disorder((4, 6, 18), (True, False, True), 7)
    s3 = tempering_scan_3d((4, 6, 18), TS, couplings=J3, field=h3, periodic=(True, False, True), n_equilibrate=10, n_measure=8,
                           measure_every=2, seed=3, replicas=2, correlation=True)
    assert s3["chi_k"].shape == (len(TS), 3) and np.isnan(s3["chi_k"][:, 1]).all() and np.isfinite(s3["chi_k"][:, [0, 2]]).all()
    assert np.isnan(s3["xi"][:, 1]).all()


def test_c_abi_errors(hip):
    pt = hip.TemperingLattice(8, 16, True, 3, 1)
    op = hip.TemperingLattice(8, 16, False, 3, 1)
    p3 = hip.TemperingLattice3D(4, 6, 16, (True, False, True), 3, 2)
    slab = hip.Lattice(32, 64, True, total_rows=64, row0=0, ghost=2)
    whole, other = hip.Lattice(32, 64, True), hip.Lattice(32, 48, True)
    t8, t16, t4 = twin.tables(8), twin.tables(16), twin.tables(4)
    try:
        with pytest.raises(ValueError, match="NULL table"):
            pt.set_correlation(True, [t8, None])
        with pytest.raises(ValueError, match="NULL table"):
            pt.set_correlation(True, None)
        with pytest.raises(ValueError, match="no periodic axis"):
            op.set_correlation(True, [None, None])
        op.set_correlation(False, None)  # off is always fine
        with pytest.raises(ValueError, match="open"):
            p3.set_correlation(True, [t4, twin.tables(6), t16])
        p3.set_correlation(True, [t4, None, t16])
        with pytest.raises(ValueError, match="recorded no modes"):
            p3.history_modes()
        with pytest.raises(ValueError, match="out of range"):
            pt.profiles(3)
        with pytest.raises(hip.UnsupportedError):
            slab.profiles()
        with pytest.raises(hip.UnsupportedError):
            whole.profiles(slab)
        with pytest.raises(ValueError, match="shapes differ"):
            whole.profiles(other)
    finally:
        for x in (pt, op, p3, slab, whole, other):
            x.close()


# ---------------------------------------------------------------- physics
ENUM_TS = [0.8, 1.2, 1.7, 2.4]
ENUM_NB = 20


def _chi_deviations(modes, axis, exact):
    """Per slot: (mean of the batch means of |F_axis|^2, exact, standard error of the mean)."""
    out = []
    for i, ex in enumerate(exact):
        b = (np.abs(modes[:, i, axis]) ** 2).reshape(ENUM_NB, -1).mean(axis=1)
        out.append((float(b.mean()), float(ex), float(b.std(ddof=1) / math.sqrt(ENUM_NB))))
    return out


@pytest.mark.parametrize("shape,periodic,axis,dseed,seed", [((4, 2, 2), (True, False, False), 0, 21, 5), ((4, 4), True, 0, 21, 5)])
def test_chi_k_against_exact_enumeration(hip, shape, periodic, axis, dseed, seed):
    """Two ladders over four temperatures on enumeration_disorder's Gaussian couplings and field (its zeroed last slices leave the
    wrap bonds at 0; the periodic flag only defines the mode): 400 discarded rounds, 8000 recorded rounds of 5 sweeps (the lengths
    of test_tempering3d_gpu's enumeration test), 20 batch means; <|F|^2> of the overlap field along `axis` at every slot within 4
    standard errors of sum_ij cos(k (x_i - x_j)) <s_i s_j>^2 from full enumeration (correlation_twin.exact_chi_k).

    Seeds (21, 5), the first pair of test_tempering3d_gpu's rehearsals, were fixed before any device run and rehearsed once on the
    CPU with tempering3d_twin / tempering_twin on their own float64 energies (the statistics, not the bits), modes from
    correlation_twin.  Deviations of the rehearsal per slot, in units of the standard error: z-periodic 4x2x2 +1.06, -1.68, +0.37,
    -1.28 (acceptance 0.59 ... 0.63, 4972 round trips); periodic 4x4 -1.00, -0.35, +1.27, -0.00 (0.55 ... 0.65, 4706).  No other seed
    was tried.  The device figures are printed by the test (run with -s).
    """
    from tsu.models.ising import LatticeTempering, LatticeTempering3D
    if len(shape) == 3:
        jr, jd, jl, h = twin.enumeration_disorder(shape, dseed)
        pt = LatticeTempering3D(shape, ENUM_TS, couplings=(jr, jd, jl), field=h, periodic=periodic, seed=seed, ladders=2, correlation=True)
        disorder = (jr, jd, jl, h)
    else:
        jr, jd, _, h = (a[0] for a in twin.enumeration_disorder((1,) + shape, dseed))
        pt = LatticeTempering(shape, ENUM_TS, couplings=(jr, jd), field=h, periodic=periodic, seed=seed, ladders=2, correlation=True)
        disorder = (jr, jd, h)
    try:
        pt.run(400, 5, record=False)
        modes = pt.run(8000, 5)["modes"]
        exact = [twin.exact_chi_k(shape, periodic, disorder, T)[axis] for T in ENUM_TS]
        worst = 0.0
        for i, (mean, ex, se) in enumerate(_chi_deviations(modes, axis, exact)):
            print(f"T={ENUM_TS[i]:.2f} <|F|^2>={mean:.6f} exact={ex:.6f} se={se:.2e} dev={(mean - ex) / se:+.2f} se")
            worst = max(worst, abs(mean - ex) / se)
            assert abs(mean - ex) < 4 * se, (i, ENUM_TS[i], mean, ex, se)
        print(f"worst deviation {worst:.2f} se")
    finally:
        pt._pt.close()


def test_ferromagnet_orders(hip):
    """3-D ferromagnet (T_c = 4.51): below it the spins order and xi_L / L of the spin field is large, above it the correlations are
    short: xi_over_L(3.5) > xi_over_L(6.0).  Qualitative; from an ordered start, so no domain walls have to heal."""
    from tsu.models.ising import temperature_scan_3d
    out = temperature_scan_3d((8, 8, 8), [3.5, 6.0], n_equilibrate=200, n_measure=100, measure_every=2, seed=1, initial="up",
                              correlation=True)
    print("xi_over_L", out["xi_over_L"], "chi_k", out["chi_k"])
    assert out["chi_k"].shape == (2, 3) and np.isfinite(out["xi_over_L"]).all()
    assert out["xi_over_L"][0] > out["xi_over_L"][1]

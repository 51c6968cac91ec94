"""Overlaps of walker pairs on the GPU (csrc/link_dev.h, tsu_hip_overlap.h): the link overlap of lattice pairs, of the slots of
two-ladder tempering handles and of a population's pairs (i, i + P), bit-exact integers against tests/helpers/overlap_twin.py; the
pairs' spin overlap and k_min modes against the lattice and correlation twins; the family mask against the device's parents;
<q^2>, <q_l> and <|F(k_min)|^2> of an annealed 16-site glass against full enumeration; C-ABI errors.

The 2-D handles take a periodic lattice only with even sides >= 4, so a periodic row whose last chunk holds a single column does not
exist: the wrap from a short last chunk to chunk 0 is taken at (6, 18) (two columns in the last chunk), the one-column last chunk
at (6, 17) open, and the 15|16 seam at (3, 32) open and (4, 32) periodic."""
import ctypes
import importlib.util
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


twin = _load("overlap_twin")
corr = _load("correlation_twin")
lattice3d_twin = corr.lattice3d_twin


@pytest.fixture(scope="module")
def hip():
    from tsu import _hip
    return _hip


def _spins(shape, seed):
    return (2 * np.random.default_rng(seed).integers(0, 2, size=shape, dtype=np.int8) - 1).astype(np.int8)


def _disorder(shape, periodic, seed, field=True):
    """Gaussian couplings (and field) of a 2-D or 3-D lattice, the last slice of an open axis's J zero (test_population_gpu's)."""
    rng = np.random.default_rng(seed)
    js = [rng.normal(size=shape).astype(np.float32) for _ in shape]  # J_right, J_down(, J_layer)
    per = twin.axes(shape, periodic)
    for j, axis in zip(js, range(len(shape) - 1, -1, -1)):
        if not per[axis]:
            np.moveaxis(j, axis, 0)[-1] = 0.0
    return tuple(js) + ((rng.normal(size=shape).astype(np.float32) if field else None),)


def _models(shape, periodic, sa, sb):
    from tsu.models import ising
    One = ising.IsingModel2D if len(shape) == 2 else ising.IsingModel3D
    a, b = One(shape, periodic=periodic, seed=1, initial="up"), One(shape, periodic=periodic, seed=2, initial="up")
    a.spins, b.spins = sa, sb
    return a, b


# ---------------------------------------------------------------- lattice pairs
PAIRS_2D = [((5, 37), False), ((16, 16), True), ((6, 17), False), ((6, 18), True), ((3, 32), False), ((4, 32), True), ((4, 4), True),
            ((1, 40), False), ((40, 1), False)]
PAIRS_3D = [((3, 4, 6), (False, True, True)), ((2, 3, 18), False), ((4, 4, 16), True), ((1, 6, 17), False), ((5, 9, 33), False),
            ((4, 12, 40), (True, False, True))]


@pytest.mark.parametrize("shape,periodic", PAIRS_2D + PAIRS_3D)
def test_lattice_pair_equals_the_twin(hip, shape, periodic):
    sa, sb = _spins(shape, 11), _spins(shape, 12)
    a, b = _models(shape, periodic, sa, sb)
    want = twin.link_overlap(sa, sb, periodic)
    assert a._lat.link_overlap(b._lat) == want
    assert b._lat.link_overlap(a._lat) == want
    assert a.link_overlap(b) == want[0] / want[1]
    assert want[1] == twin.bond_count(shape, periodic)


def test_one_layer_equals_the_2d_lattice(hip):
    sa, sb = _spins((1, 6, 17), 13), _spins((1, 6, 17), 14)
    a3, b3 = _models((1, 6, 17), False, sa, sb)
    a2, b2 = _models((6, 17), False, sa[0], sb[0])
    assert a3._lat.link_overlap(b3._lat) == a2._lat.link_overlap(b2._lat) == twin.link_overlap(sa[0], sb[0], False)
    sa, sb = _spins((1, 8, 36), 15), _spins((1, 8, 36), 16)  # and with the in-layer wraps
    a3, b3 = _models((1, 8, 36), (False, True, True), sa, sb)
    a2, b2 = _models((8, 36), True, sa[0], sb[0])
    assert a3._lat.link_overlap(b3._lat) == a2._lat.link_overlap(b2._lat) == twin.link_overlap(sa[0], sb[0], True)


def test_a_plane_with_more_lanes_than_the_grid_holds(hip):
    """4100 x 8200 open: 513 bands of 8 rows x 513 chunks = 263 169 lanes against the 1024 x 256 = 262 144 of the capped grid, so
    the last lanes are reached by the grid-stride loop."""
    shape = (4100, 8200)
    sa, sb = _spins(shape, 17), _spins(shape, 18)
    a, b = _models(shape, False, sa, sb)
    assert a._lat.link_overlap(b._lat) == twin.link_overlap(sa, sb, False)


@pytest.mark.parametrize("shape,periodic", [((6, 18), True), ((5, 37), False), ((3, 4, 6), (False, True, True)), ((4, 4, 16), True)])
def test_identities_through_the_c_abi(hip, shape, periodic):
    sa = _spins(shape, 19)
    a, b = _models(shape, periodic, sa, -sa)
    nb = twin.bond_count(shape, periodic)
    lib = a._lat.lib
    fn = lib.tsu_ising2d_link_overlap if len(shape) == 2 else lib.tsu_ising3d_link_overlap
    for x, y in ((a, a), (a, b), (b, a)):  # b == a is accepted: L(a, a) = L(a, -a) = N_b
        L, n = ctypes.c_int64(-1), ctypes.c_int64(-1)
        assert fn(x._lat.h, y._lat.h, ctypes.byref(L), ctypes.byref(n)) == hip.TSU_OK
        assert (L.value, n.value) == (nb, nb)
    flip = sa.copy()
    site = tuple(n // 2 for n in shape)
    flip[site] = -flip[site]
    b.spins = flip
    assert a._lat.link_overlap(b._lat) == (nb - 2 * twin.degree(shape, periodic, site), nb)


# ---------------------------------------------------------------- ladders
@pytest.mark.parametrize("shape,periodic,n_temps", [((12, 20), False, 5), ((3, 4, 6), (False, True, True), 4)])
def test_ladders_record_the_link_overlap_per_slot(hip, shape, periodic, n_temps):
    from tsu.models import ising
    PT = ising.LatticeTempering if len(shape) == 2 else ising.LatticeTempering3D
    dis = _disorder(shape, periodic, 31)
    Ts = list(np.linspace(0.8, 3.0, n_temps))
    kw = dict(couplings=dis[:-1], field=dis[-1], periodic=periodic, seed=77, ladders=2)
    on, off = PT(shape, Ts, link_overlap=True, **kw), PT(shape, Ts, **kw)
    Handle = hip.TemperingLattice if len(shape) == 2 else hip.TemperingLattice3D
    raw = Handle(*shape, periodic, n_temps, 2)  # switched on and off again before its first run
    raw.set_disorder(*dis)
    raw.set_temperatures(Ts)
    raw.set_link_overlap(True)
    raw.set_link_overlap(False)
    raw.init(77, 0)
    try:
        swapped = False
        for _ in range(3):
            h, h_off = on.run(1, 2), off.run(1, 2)
            raw.run(1, 2)
            h_raw = raw.history()
            assert "q_link" not in h_off and "q_link" not in h_raw
            assert h["q_link"].shape == (1, n_temps) and h["q_link"].dtype == np.int64
            for slot in range(n_temps):
                a, b = on.spins(slot, 0), on.spins(slot, 1)
                assert int(h["q_link"][0, slot]) == twin.link_overlap(a, b, periodic)[0], slot
                assert int(h["q"][0, slot]) == lattice3d_twin.overlap(a, b)
            for key in ("E", "M", "walker", "q"):  # the switch leaves the chain what it was
                assert (h[key] == h_off[key]).all(), key
            assert (h_raw["q"] == h["q"]).all() and (h_raw["E"][:, 0] == h["E"]).all()
            swapped = swapped or (on.walker_at_slot != np.arange(n_temps)).any()
        assert swapped, "no swap was accepted: the slots still hold their first walkers"
        assert on._pt.launch_count() == off._pt.launch_count() == raw.launch_count() == 2 * 2 * 3
    finally:
        for x in (on._pt, off._pt, raw):
            x.close()


def test_tempering_scans_report_the_link_overlap(hip):
    from tsu.models import ising
    Ts = [1.0, 2.0, 4.0]
    dis = _disorder((8, 16), True, 32, field=False)
    kw = dict(couplings=dis[:2], n_equilibrate=4, n_measure=5, measure_every=2, seed=3, replicas=2)
    out = ising.tempering_scan((8, 16), Ts, link_overlap=True, **kw)
    plain = ising.tempering_scan((8, 16), Ts, **kw)
    assert "link_overlap" not in plain and out["link_overlap"].shape == (3,) and (np.abs(out["link_overlap"]) <= 1).all()
    np.testing.assert_array_equal(out["overlap_sq"], plain["overlap_sq"])
    pt = ising.LatticeTempering((8, 16), Ts, couplings=dis[:2], seed=3, initial="up", ladders=2, link_overlap=True)
    try:
        pt.run(2, 2, record=False)
        h = pt.run(5, 2)
    finally:
        pt._pt.close()
    np.testing.assert_array_equal(out["link_overlap"], h["q_link"].mean(axis=0) / twin.bond_count((8, 16), True))
    dis3 = _disorder((2, 4, 16), (False, True, True), 33, field=False)
    out3 = ising.tempering_scan_3d((2, 4, 16), Ts, couplings=dis3[:3], periodic=(False, True, True), n_equilibrate=2, n_measure=3,
                                   measure_every=1, seed=4, replicas=2, link_overlap=True)
    assert out3["link_overlap"].shape == (3,) and out3["link_overlap"][0] > out3["link_overlap"][2]  # 'up' start, cold stays ordered


# ---------------------------------------------------------------- populations, step by step
def _handle(hip, shape, periodic, R, dis, betas, seed, correlation=True):
    pa = (hip.PopulationLattice if len(shape) == 2 else hip.PopulationLattice3D)(*shape, periodic, R)
    pa.set_disorder(*dis)
    pa.set_schedule(betas)
    per = twin.axes(shape, periodic)
    pa.set_overlap(True, [corr.tables(n) if p else None for n, p in zip(shape, per)] if correlation else None)
    pa.init(seed, 0)
    return pa


def _planes(pa):
    return np.stack([pa.get_spins(i) for i in range(pa.population)])


def _twin_rows(planes, periodic):
    """(q, L, modes over the periodic axes) of the pairs of `planes`, by the twins."""
    per = np.array(twin.axes(planes.shape[1:], periodic))
    q, L = twin.pair_rows(planes, periodic)
    modes = np.array([corr.modes(corr.profiles(planes[i], planes[j]), per)[per] for i, j in twin.pairs(planes.shape[0])])
    return q, L, modes.reshape(len(q), int(per.sum()))


def _stepwise(hip, shape, periodic, R, dis, betas, seed, theta):
    """One recorded step per call, all planes read back after each: rows 0 and 1 of every call against the twins on the planes
    before and after.  Returns the joined record."""
    pa = _handle(hip, shape, periodic, R, dis, betas, seed)
    try:
        rows = [_twin_rows(_planes(pa), periodic)]
        parents = []
        for j in range(len(betas) - 1):
            pa.run(1, theta)
            rec = pa.history()
            rows.append(_twin_rows(_planes(pa), periodic))
            for r in (0, 1):
                q, L, modes = rows[j + r]
                assert (rec["q"][r] == q).all() and (rec["q_link"][r] == L).all(), (j, r)
                assert rec["modes"][r].shape == modes.shape
                assert (rec["modes"][r].real == modes.real).all() and (rec["modes"][r].imag == modes.imag).all(), (j, r)  # bit for bit
            parents.append(rec["parent"][0])
        assert pa.launch_count() == 2 * theta * (len(betas) - 1)  # half-sweeps only, as without the switch
    finally:
        pa.close()
    return {"parent": np.array(parents), "q": np.array([r[0] for r in rows]), "q_link": np.array([r[1] for r in rows]),
            "modes": np.array([r[2] for r in rows])}


STEP_BETAS = [0.0, 1.0, 2.0, 3.0, 4.0]
# Same-family pairs of 32 per step at R = 65, from a pure-NumPy run of this schedule (population_twin's resampler and sweeps on the
# lattice twin's energies, overlap_twin's mask): (4, 4) has both kinds of pair at every step after the start; on (4, 2, 2) the
# walkers that die at step 1 all copy a walker outside their own pair, so both kinds are there from step 2 on.
SAME_FAMILY_65 = {(4, 4): [0, 4, 9, 14, 14], (4, 2, 2): [0, 0, 5, 9, 11]}


@pytest.mark.parametrize("R", [2, 3, 65, 1025])
@pytest.mark.parametrize("shape,periodic", [((4, 4), True), ((4, 2, 2), (True, False, False))])
def test_population_rows_equal_the_twins_step_by_step(hip, shape, periodic, R):
    from tsu.models import ising
    seed, theta = 5, 2
    dis = _disorder(shape, periodic, 21, field=False)
    rec = _stepwise(hip, shape, periodic, R, dis, STEP_BETAS, seed, theta)
    mask = twin.pair_mask(rec["parent"])
    N, nb = int(np.prod(shape)), twin.bond_count(shape, periodic)
    st = ising.population_overlap_stats(rec["parent"], rec["q"], rec["q_link"], N, nb)
    assert (st["pairs"] == mask.sum(axis=1)).all() and st["pairs"][0] == R // 2
    same = (~mask).sum(axis=1)
    print(f"{shape} R={R}: same-family pairs per step {same.tolist()} of {R // 2}")
    if R == 65:  # both kinds of pair are there, so the mask is tested both ways
        assert same.tolist() == SAME_FAMILY_65[shape]
        first = 1 if shape == (4, 4) else 2
        assert ((same[first:] > 0) & (mask.sum(axis=1)[first:] > 0)).all()
    if R == 2:  # the single pair falls into one family at step 1
        assert (st["pairs"][1:] == 0).all()
        for key in ("overlap", "overlap_sq", "binder", "link_overlap"):
            assert np.isnan(st[key][1:]).all(), key
        assert st["overlap_sq"][0] == (rec["q"][0, 0] / N) ** 2
    # the same schedule in one call, and split 1 + 3, through the model layer: the same rows, and overlap_stats of the record
    Pop = ising.PopulationAnnealing if len(shape) == 2 else ising.PopulationAnnealing3D
    kw = dict(betas=STEP_BETAS, couplings=dis[:-1], periodic=periodic, seed=seed, sweeps_per_step=theta, overlap=True, correlation=True)
    one, two = Pop(shape, R, **kw), Pop(shape, R, **kw)
    try:
        h1 = one.run()
        two.run(1)
        h2 = two.run()
        per = np.array(twin.axes(shape, periodic))
        for key in h1:
            assert np.array_equal(h1[key], h2[key], equal_nan=True), key
        assert (h1["parent"] == rec["parent"]).all() and (h1["q"] == rec["q"]).all() and (h1["q_link"] == rec["q_link"]).all()
        assert np.array_equal(h1["modes"][:, :, per], rec["modes"]) and np.isnan(h1["modes"][:, :, ~per]).all()
        got = one.overlap_stats()
        assert (got["pairs"] == mask.sum(axis=1)).all()
        for key in ("overlap", "overlap_sq", "binder", "link_overlap"):
            np.testing.assert_array_equal(got[key], st[key])
        assert got["chi_k"].shape == (5, len(shape)) and got["xi_over_L"].shape == (5,)
        hist = one.overlap_histogram(8)
        assert (hist["pairs"] == got["pairs"]).all() and hist["P"].shape == (5, 8)
        ok = got["pairs"] > 0
        np.testing.assert_allclose(hist["P"][ok].sum(axis=1) * 0.25, 1.0, rtol=1e-12)
        assert np.isnan(hist["P"][~ok]).all()
    finally:
        one._pa.close()
        two._pa.close()


def test_population_rows_on_a_plane_of_several_chunks(hip):
    """(8, 24) periodic, R = 65, correlation on: two chunks a row, the second of 8 columns, both wraps."""
    shape, periodic = (8, 24), True
    dis = _disorder(shape, periodic, 21, field=False)
    rec = _stepwise(hip, shape, periodic, 65, dis, [0.0, 0.2, 0.4, 0.6], 5, 2)
    assert (rec["parent"] != np.arange(65)).any() and (np.abs(rec["q"]) < 8 * 24).all()


def test_overlap_without_tables_records_q_and_l_only(hip):
    shape, periodic = (4, 2, 2), (True, False, False)
    dis = _disorder(shape, periodic, 21, field=False)
    pa = _handle(hip, shape, periodic, 9, dis, STEP_BETAS, 5, correlation=False)
    try:
        pa.run(2, 1)
        rec = pa.history()
        assert "modes" not in rec and rec["q"].shape == (3, 4)
        q, L = twin.pair_rows(_planes(pa), periodic)
        assert (rec["q"][2] == q).all() and (rec["q_link"][2] == L).all()
        pa.run(1, 1, record=False)
        with pytest.raises(ValueError, match="recorded nothing"):
            pa.history()
    finally:
        pa.close()


def test_population_scans_add_the_overlap_keys(hip):
    from tsu.models import ising
    dis = _disorder((8, 8), True, 2, field=False)
    kw = dict(betas=np.linspace(0.0, 1.0, 6), couplings=dis[:2], seed=3, sweeps_per_step=2)
    plain = ising.population_annealing_scan(8, 300, **kw)
    out = ising.population_annealing_scan(8, 300, overlap=True, correlation=True, **kw)
    for key in plain:  # every existing key, unchanged
        np.testing.assert_array_equal(out[key], plain[key])
    assert sorted(set(out) - set(plain)) == ["binder", "chi_k", "link_overlap", "overlap", "overlap_sq", "pairs", "xi", "xi_over_L"]
    assert out["pairs"][0] == 150 and out["chi_k"].shape == (6, 2) and out["overlap_sq"].shape == (6,)
    only = ising.population_annealing_scan(8, 300, overlap=True, **kw)
    assert sorted(set(only) - set(plain)) == ["binder", "link_overlap", "overlap", "overlap_sq", "pairs"]
    np.testing.assert_array_equal(only["link_overlap"], out["link_overlap"])
    out3 = ising.population_annealing_scan_3d((2, 4, 4), 100, temperatures=[np.inf, 4.0, 2.0], periodic=(False, True, True), seed=1,
                                              sweeps_per_step=1, overlap=True, correlation=True)
    assert out3["chi_k"].shape == (3, 3) and np.isnan(out3["chi_k"][:, 0]).all() and np.isfinite(out3["chi_k"][:, 1:]).all()


# ---------------------------------------------------------------- equilibrium against full enumeration
ENUM_BETAS = np.linspace(0.0, 2.0, 21)
ENUM_CASES = [((4, 4), True), ((4, 2, 2), (True, False, False))]
ENUM_AT = [10, 15, 20]  # beta = 1.0, 1.5, 2.0


def _exact(shape, periodic, dis, beta):
    """(<q^2>, <q_l>, <|F_d|^2> per axis) of two independent replicas at beta, from C_ij = <s_i s_j> by enumeration."""
    disorder = dis[:-1] + (None,)
    C2 = corr.exact_spin_correlations(shape, periodic, disorder, 1.0 / beta) ** 2
    N = C2.shape[0]
    idx = np.arange(N).reshape(shape)
    per = twin.axes(shape, periodic)
    bonds = []
    for d, p in enumerate(per):  # the energy's bonds: every site and its successor, the wrap of a periodic axis included
        nxt = np.roll(idx, -1, axis=d)
        i, j = (idx, nxt) if p else (np.delete(idx, -1, axis=d), np.delete(nxt, -1, axis=d))
        bonds += list(zip(i.ravel(), j.ravel()))
    assert len(bonds) == twin.bond_count(shape, periodic)
    ql = float(np.mean([C2[i, j] for i, j in bonds]))
    return float(C2.sum()) / N ** 2, ql, corr.exact_chi_k(shape, periodic, disorder, 1.0 / beta)


@pytest.mark.parametrize("shape,periodic", ENUM_CASES)
def test_equilibrium_against_full_enumeration(hip, shape, periodic):
    """16-site Gaussian glass (disorder seed 21), betas = linspace(0, 2, 21), R = 4096, theta = 2, 8 seeds 10^6 apart, overlap and
    correlation on: at beta = 1.0, 1.5 and 2.0 the mean over the seeds of overlap_stats()'s <q^2>, <q_l> and <|F(k_min)|^2> of every
    periodic axis lies within 4 standard errors (of those 8 runs) + 1e-12 of sum_ij C_ij^2 / N^2, the mean of C_ij^2 over the
    energy's bonds and sum_ij C_ij^2 cos(k (x_i - x_j)), C_ij = <s_i s_j> by enumeration.  As a control, the same seeds annealed
    without resampling must miss <q^2> at beta = 2 by more than those 4 errors.  The figures of a device run are in DESIGN.md
    section 5."""
    from tsu.models import ising
    Pop = ising.PopulationAnnealing if len(shape) == 2 else ising.PopulationAnnealing3D
    dis = _disorder(shape, periodic, 21, field=False)
    per = np.array(twin.axes(shape, periodic))
    N = int(np.prod(shape))
    exact = [_exact(shape, periodic, dis, ENUM_BETAS[k]) for k in ENUM_AT]
    runs = {"q2": [], "ql": [], "F2": [], "q2_plain": [], "pairs": []}
    for seed in range(8):
        for resample in (True, False):
            pa = Pop(shape, 4096, betas=ENUM_BETAS, couplings=dis[:-1], periodic=periodic, seed=10 ** 6 * (seed + 1), sweeps_per_step=2,
                     overlap=True, correlation=True)
            try:
                pa.run(resample=resample)
                st = pa.overlap_stats()
            finally:
                pa._pa.close()
            if resample:
                runs["q2"].append(st["overlap_sq"][ENUM_AT])
                runs["ql"].append(st["link_overlap"][ENUM_AT])
                runs["F2"].append((st["chi_k"] * N)[ENUM_AT][:, per])
                runs["pairs"].append(st["pairs"])
            else:
                assert (st["pairs"] == 2048).all()
                runs["q2_plain"].append(st["overlap_sq"][ENUM_AT])
    print(f"{shape}: valid pairs of 2048, fewest per step over the seeds: {np.min(runs['pairs'], axis=0).tolist()}")
    want = {"q2": np.array([e[0] for e in exact]), "ql": np.array([e[1] for e in exact]),
            "F2": np.array([e[2][per] for e in exact])}
    failures = []
    for name in ("q2", "ql", "F2"):
        got = np.array(runs[name])
        mean, se = got.mean(axis=0), got.std(axis=0, ddof=1) / np.sqrt(8)
        dev = np.abs(mean - want[name]) / np.where(se > 0, se, 1.0)
        print(f"{shape} {name}: mean {mean.tolist()} exact {want[name].tolist()} deviation in s.e. {np.round(dev, 2).tolist()}")
        if not (np.abs(mean - want[name]) <= 4 * se + 1e-12).all():
            failures.append((name, mean, want[name], se))
    assert not failures, failures
    got = np.array(runs["q2"])
    se2 = got.std(axis=0, ddof=1)[-1] / np.sqrt(8)
    plain = np.array(runs["q2_plain"]).mean(axis=0)[-1]
    miss = abs(plain - want["q2"][-1])
    print(f"{shape} control without resampling: <q^2> at beta = 2 is {plain:.4f} against {want['q2'][-1]:.4f}: {miss / se2:.1f} s.e.")
    assert miss > 4 * se2, "the control agrees with the enumeration: the test has no power"


# ---------------------------------------------------------------- C-ABI errors, other handles
def _last_error(handle):
    return handle.lib.tsu_last_error(handle.ctx.h).decode()


def test_c_abi_errors(hip):
    i64p, f64p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    z = np.zeros((4, 4), np.float32)
    q = np.zeros((8, 8), np.int64)
    qp = q.ctypes.data_as(i64p)
    tab = [np.ascontiguousarray(t).ctypes.data_as(f64p) for t in corr.tables(4)]
    pa = hip.PopulationLattice(4, 4, True, 4)
    try:
        pa.set_disorder(z, z)
        pa.set_schedule([0.0, 1.0, 2.0])
        pa.init(1)
        pa.run(1, 1)  # recorded, overlaps off
        assert "q" not in pa.history()
        assert pa.lib.tsu_pa2d_history_overlap(pa.h, qp, qp, None) == hip.TSU_E_INVALID
        assert "pa2d_history_overlap: the last run recorded no overlaps" in _last_error(pa)
        pa.set_overlap(True)
        assert pa.lib.tsu_pa2d_history_overlap(pa.h, qp, qp, None) == hip.TSU_E_INVALID  # switching it on dropped the rows
        pa.run(1, 1, record=False)
        assert pa.lib.tsu_pa2d_history_overlap(pa.h, qp, qp, None) == hip.TSU_E_INVALID
        assert "recorded no overlaps" in _last_error(pa)
        # a NULL table of a periodic axis
        assert pa.lib.tsu_pa2d_set_overlap(pa.h, 1, tab[0], tab[1], None, None) == hip.TSU_E_INVALID
        assert "pa2d_set_overlap: NULL table of periodic axis 1" in _last_error(pa)
    finally:
        pa.close()
    po = hip.PopulationLattice(4, 4, False, 4)
    try:
        assert po.lib.tsu_pa2d_set_overlap(po.h, 1, tab[0], tab[1], tab[0], tab[1]) == hip.TSU_E_INVALID
        assert "pa2d_set_overlap: the lattice has no periodic axis" in _last_error(po)
        assert po.lib.tsu_pa2d_set_overlap(po.h, 1, None, None, None, None) == hip.TSU_OK  # q and L need no periodic axis
    finally:
        po.close()
    p3 = hip.PopulationLattice3D(4, 2, 2, (True, False, False), 4)
    try:
        assert p3.lib.tsu_pa3d_set_overlap(p3.h, 1, tab[0], tab[1], tab[0], tab[1], None, None) == hip.TSU_E_INVALID
        assert "pa3d_set_overlap: axis 1 is open: its tables must be NULL" in _last_error(p3)
        with pytest.raises(ValueError, match="axis 1 is open"):
            p3.set_overlap(True, [corr.tables(4), corr.tables(2), None])
        p3.set_overlap(True, [corr.tables(4), None, None])
    finally:
        p3.close()
    for Handle, shape, name in ((hip.TemperingLattice, (4, 4), "pt2d"), (hip.TemperingLattice3D, (4, 4, 4), "pt3d")):
        pt = Handle(*shape, True, 3, 1)
        try:
            assert getattr(pt.lib, f"tsu_{name}_set_link_overlap")(pt.h, 1) == hip.TSU_E_INVALID
            assert f"{name}_set_link_overlap: the link overlap needs two ladders" in _last_error(pt)
            assert getattr(pt.lib, f"tsu_{name}_history_link")(pt.h, qp) == hip.TSU_E_INVALID
            assert f"{name}_history_link: the last run recorded no link overlap" in _last_error(pt)
            with pytest.raises(ValueError, match="two ladders"):
                pt.set_link_overlap(True)
        finally:
            pt.close()
    L, n = ctypes.c_int64(0), ctypes.c_int64(0)
    a, b, c = hip.Lattice(4, 16, False), hip.Lattice(4, 32, False), hip.Lattice(4, 16, True)
    slab = hip.Lattice(4, 16, False, total_rows=8, row0=0, ghost=2)
    try:
        assert a.lib.tsu_ising2d_link_overlap(a.h, b.h, ctypes.byref(L), ctypes.byref(n)) == hip.TSU_E_INVALID
        assert "ising2d_link_overlap: shapes differ (4 x 16 against 4 x 32)" in _last_error(a)
        assert a.lib.tsu_ising2d_link_overlap(a.h, c.h, ctypes.byref(L), ctypes.byref(n)) == hip.TSU_E_INVALID
        assert "one lattice is periodic and the other is open" in _last_error(a)
        for x, y in ((a, slab), (slab, a), (slab, slab)):
            assert a.lib.tsu_ising2d_link_overlap(x.h, y.h, ctypes.byref(L), ctypes.byref(n)) == hip.TSU_E_UNSUPPORTED
            assert "ising2d_link_overlap: whole lattices only (not slabs)" in _last_error(a)
        with pytest.raises(hip.UnsupportedError, match="whole lattices only"):
            a.link_overlap(slab)
    finally:
        for x in (a, b, c, slab):
            x.close()
    a3, b3, c3 = hip.Lattice3D(2, 4, 16, False), hip.Lattice3D(2, 4, 32, False), hip.Lattice3D(2, 4, 16, (False, True, False))
    try:
        assert a3.lib.tsu_ising3d_link_overlap(a3.h, b3.h, ctypes.byref(L), ctypes.byref(n)) == hip.TSU_E_INVALID
        assert "ising3d_link_overlap: shapes differ (2 x 4 x 16 against 2 x 4 x 32)" in _last_error(a3)
        assert a3.lib.tsu_ising3d_link_overlap(a3.h, c3.h, ctypes.byref(L), ctypes.byref(n)) == hip.TSU_E_INVALID
        assert "the periodic axes of the two lattices differ" in _last_error(a3)
    finally:
        for x in (a3, b3, c3):
            x.close()


def test_other_handles_are_untouched_beside_a_population_with_overlaps(hip):
    from tsu.models import ising
    dis = _disorder((8, 16), True, 4)
    Ts = [0.8, 1.6, 3.2]

    def others():
        one = ising.IsingModel2D((8, 16), temperature=1.1, seed=5, couplings=dis[:2], field=dis[2])
        one.gibbs_update(4)
        pt = ising.LatticeTempering((8, 16), Ts, couplings=dis[:2], field=dis[2], seed=6, ladders=2)
        h = pt.run(6, 2)
        out = (one.spins, one.energy(), h["E"].copy(), h["walker"].copy(), [pt.spins(w) for w in range(3)], h["q"].copy())
        pt._pt.close()
        return out
    want = others()
    pa = _handle(hip, (8, 16), True, 50, dis, [0.0, 0.5, 1.0], 5)
    plain = hip.PopulationLattice(8, 16, True, 50)
    plain.set_disorder(*dis)
    plain.set_schedule([0.0, 0.5, 1.0])
    plain.init(5)
    try:
        pa.run(1, 2)
        got = others()
        pa.run(1, 2)
        plain.run(2, 2)
        assert (_planes(pa) == _planes(plain)).all()  # nor does the switch change the population's own chain
        hp = plain.history()
        assert "q" not in hp and (pa.history()["E"][-1] == hp["E"][-1]).all() and pa.launch_count() == plain.launch_count()
    finally:
        pa.close()
        plain.close()
    assert (got[0] == want[0]).all() and got[1] == want[1] and (got[2] == want[2]).all() and (got[3] == want[3]).all()
    assert all((g == w).all() for g, w in zip(got[4], want[4])) and (got[5] == want[5]).all()

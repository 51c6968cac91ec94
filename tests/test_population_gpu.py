"""Population annealing on the GPU (tsu_pa2d_* / tsu_pa3d_*, csrc/pop_dev.h, csrc/pop_host.h): without resampling a walker is the
single lattice with its seed bit for bit; with it, every step's weights, offset, counts, parents and planes equal the twin's
(tests/helpers/population_twin.py, fed the device's energies and weights) across the plan's wave, workgroup and chunk boundaries and
on awkward planes; ln Z and <E> against full enumeration; determinism, accounting and C-ABI errors."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("population_twin", os.path.join(HERE, "helpers", "population_twin.py"))
twin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(twin)


@pytest.fixture(scope="module")
def hip():
    from tsu import _hip
    return _hip


def _disorder(shape, periodic, seed, field=True):
    """Gaussian couplings (and field) of a 2-D or 3-D lattice, the last slice of an open axis's J zero."""
    rng = np.random.default_rng(seed)
    js = [rng.normal(size=shape).astype(np.float32) for _ in shape]  # J_right, J_down(, J_layer)
    per = (bool(periodic),) * 2 if len(shape) == 2 else twin.lattice3d_twin.axes(periodic)
    for j, axis in zip(js, range(len(shape) - 1, -1, -1)):
        if not per[axis]:
            np.moveaxis(j, axis, 0)[-1] = 0.0
    return tuple(js) + ((rng.normal(size=shape).astype(np.float32) if field else None),)


def _handle(hip, shape, periodic, R, dis, betas, seed, initial_sweeps=0):
    pa = (hip.PopulationLattice if len(shape) == 2 else hip.PopulationLattice3D)(*shape, periodic, R)
    pa.set_disorder(*dis)
    pa.set_schedule(betas)
    pa.init(seed, initial_sweeps)
    return pa


def _planes(pa):
    return np.stack([pa.get_spins(i) for i in range(pa.population)])


def _model(shape):
    from tsu.models import ising
    return (ising.PopulationAnnealing, ising.IsingModel2D) if len(shape) == 2 else (ising.PopulationAnnealing3D, ising.IsingModel3D)


# ---------------------------------------------------------------- resample=False: the single lattices, bit for bit
@pytest.mark.parametrize("shape,periodic", [((12, 20), False), ((16, 16), True), ((3, 4, 6), (False, True, True)), ((3, 4, 6), False)])
@pytest.mark.parametrize("betas,initial_sweeps", [([0.0, 0.3, 0.7, 1.2], 0), ([0.4, 0.9, 1.5, 1.6], 3)])
def test_without_resampling_walkers_are_the_single_lattices(hip, shape, periodic, betas, initial_sweeps):
    R, theta, seed = 5, 2, (1 << 32) - 2  # seed + i carries into the key's high word
    Pop, One = _model(shape)
    dis = _disorder(shape, periodic, 11 + shape[-1])
    pa = Pop(shape, R, betas=betas, couplings=dis[:-1], field=dis[-1], periodic=periodic, seed=seed, sweeps_per_step=theta,
             initial_sweeps=initial_sweeps)
    try:
        h = pa.run(resample=False)
        assert h["E"].shape == (4, R) and (h["parent"] == np.arange(R)).all() and not h["W"].any() and not h["resampled"].any()
        assert pa.sweep_count == initial_sweeps + 3 * theta and pa.step_count == 3
        E_now = pa.energies()
        for i in range(R):
            one = One(shape, temperature=1.0 / betas[1], periodic=periodic, seed=seed + i, couplings=dis[:-1], field=dis[-1])
            rows = []
            if initial_sweeps:
                one.equilibrate(1.0 / betas[0], initial_sweeps)
            rows.append((one.energy(), round(one.magnetization() * one.n_spins)))
            for k in range(1, 4):
                one.equilibrate(1.0 / betas[k], theta)
                rows.append((one.energy(), round(one.magnetization() * one.n_spins)))
            assert (pa.spins(i) == one.spins).all(), f"walker {i} differs from the single lattice with seed + {i}"
            assert [float(x) for x in h["E"][:, i]] == [e for e, _ in rows]  # bit for bit
            assert [int(x) for x in h["M"][:, i]] == [m for _, m in rows]
            assert E_now[i] == rows[-1][0]
    finally:
        pa._pa.close()


# ---------------------------------------------------------------- the chain against the twin
def _check_chain_stepwise(pa, shape, periodic, dis, betas, seed, theta):
    """Checks (a)-(c) step by step: one recorded step per call, all planes read back after each.  Returns the died fractions."""
    R = pa.population
    before = _planes(pa)
    assert (before == twin.initial_spins(shape, seed, R)).all(), "initial draw"
    died = []
    for j in range(len(betas) - 1):
        pa.run(1, theta, resample=True, record=True)
        rec = pa.history()
        after = _planes(pa)
        died += twin.check_chain(betas, seed, theta, periodic, dis, before, rec, [after], step0=j, sweep0=j * theta)
        E, M = pa.energies()
        assert (E == rec["E"][1]).all() and (M == rec["M"][1]).all()
        assert (M == after.reshape(R, -1).sum(axis=1, dtype=np.int64)).all()
        before = after
    return died


@pytest.mark.parametrize("R", [2, 3, 64, 65, 257, 1025, 4097])
@pytest.mark.parametrize("db", [1e-9, 0.3, 5.0])
def test_plan_across_its_boundaries(hip, R, db):
    """4 x 4 Gaussian glass, four steps of db from beta = 0: R around a wave (64), the workgroup (1024) and several walkers per
    thread (4097), from nobody dying (db = 1e-9) to a few walkers taking almost everything (db = 5)."""
    shape, periodic, seed, theta = (4, 4), True, 4242, 1
    dis = _disorder(shape, periodic, 3, field=False)
    betas = [db * k for k in range(5)]
    pa = _handle(hip, shape, periodic, R, dis, betas, seed)
    try:
        died = _check_chain_stepwise(pa, shape, periodic, dis, betas, seed, theta)
        print(f"R={R} db={db}: died per step {['%.3f' % d for d in died]}")
        assert pa.launch_count() == 2 * theta * 4
        if db == 1e-9:
            assert died == [0.0] * 4
        if db == 5.0 and R >= 64:
            assert died[0] > 0.5
    finally:
        pa.close()


@pytest.mark.parametrize("shape,periodic", [((5, 37), False), ((64, 64), True), ((3, 5, 18), False)])
def test_copy_on_awkward_planes(hip, shape, periodic):
    """The full chain for three steps, R = 33, theta = 1: planes of one 16-byte chunk per row with pad columns, of whole 256-byte
    rows, and of 3-D rows of two chunks."""
    R, seed, theta = 33, 99, 1
    dis = _disorder(shape, periodic, 5 + shape[0])
    betas = [0.0, 0.05, 0.1, 0.15] if shape == (64, 64) else [0.0, 0.3, 0.6, 0.9]
    pa = _handle(hip, shape, periodic, R, dis, betas, seed)
    try:
        died = _check_chain_stepwise(pa, shape, periodic, dis, betas, seed, theta)
        print(f"{shape}: died per step {['%.3f' % d for d in died]}")
        assert max(died) > 0, "no plane was copied: the case checks nothing"
    finally:
        pa.close()


# ---------------------------------------------------------------- equilibrium against full enumeration
ENUM_BETAS = np.linspace(0.0, 2.0, 21)
ENUM_CASES = [((4, 4), True), ((4, 2, 2), (True, False, False))]


def _enumerate(shape, periodic, dis, betas):
    """(ln Z, <E>) at every beta by enumerating the 2^16 states (zero field)."""
    n = int(np.prod(shape))
    idx = np.arange(1 << n, dtype=np.int64)
    S = np.stack([1 - 2 * ((idx >> k) & 1) for k in range(n)], axis=1).astype(np.float64).reshape((1 << n,) + tuple(shape))
    per = (bool(periodic),) * 2 if len(shape) == 2 else twin.lattice3d_twin.axes(periodic)
    E = np.zeros(1 << n)
    for j, axis in zip(dis[:-1], range(len(shape) - 1, -1, -1)):  # J_right: last axis, J_down: the one before, ..
        t = j.astype(np.float64)[None] * S * np.roll(S, -1, axis=axis + 1)
        if not per[axis]:
            t = np.delete(t, -1, axis=axis + 1)
        E -= t.reshape(1 << n, -1).sum(axis=1)
    lnZ, meanE = [], []
    for b in betas:
        a = -b * E
        w = np.exp(a - a.max())
        lnZ.append(a.max() + np.log(w.sum()))
        meanE.append(float((w * E).sum() / w.sum()))
    return np.array(lnZ), np.array(meanE)


@pytest.mark.parametrize("shape,periodic", ENUM_CASES)
def test_equilibrium_against_full_enumeration(hip, shape, periodic):
    """16-site Gaussian glass, betas = linspace(0, 2, 21), R = 4096, theta = 2, 8 seeds 10^6 apart (walker i has key
    seed + i: seeds closer than R would share keys, hence starts and uniforms, between the runs, and their spread would understate
    the error): the mean over the seeds of ln Z and of
    <E> at every beta within 4 standard errors (of those 8 runs) of the enumerated value; 1e-12 is added to the bound for the
    rounding of the enumeration's own float64 sums (at beta = 0 every run gives N ln 2 and the standard error is 0).  As a control,
    the same estimator on the records of the same 8 seeds annealed without resampling must miss ln Z at the last beta by more than
    those 4 errors.  The figures of a device run are in DESIGN.md section 5."""
    Pop, _ = _model(shape)
    dis = _disorder(shape, periodic, 21, field=False)
    exact_lnZ, exact_E = _enumerate(shape, periodic, dis, ENUM_BETAS)
    R, n = 4096, int(np.prod(shape))
    lnZ, meanE, lnZ_plain, died = [], [], [], []
    for seed in range(8):
        for resample in (True, False):
            pa = Pop(shape, R, betas=ENUM_BETAS, couplings=dis[:-1], periodic=periodic, seed=10 ** 6 * (seed + 1), sweeps_per_step=2)
            try:
                h = pa.run(resample=resample)
                if resample:
                    lnZ.append(pa.free_energy()["ln_Z"])
                    meanE.append(pa.observables()["energy"])
                    died.append((h["parent"] != np.arange(R)).mean(axis=1))
                else:  # the weights the walkers would have had, from the recorded energies: nobody was resampled
                    S, Emin = zip(*[(sum(w), e) for w, e in (twin.weights(h["E"][k], ENUM_BETAS[k + 1] - ENUM_BETAS[k]) for k in range(20))])
                    from tsu.models.ising import population_free_energy
                    lnZ_plain.append(population_free_energy(ENUM_BETAS, S, Emin, h["E"].mean(axis=1), R, n)["ln_Z"])
            finally:
                pa._pa.close()
    died = np.array(died)
    print(f"{shape}: died per step mean {died.mean():.3f} max {died.max():.3f}")
    worst = {}
    for name, runs, exact in (("ln Z", np.array(lnZ), exact_lnZ), ("<E>", np.array(meanE), exact_E)):
        mean, se = runs.mean(axis=0), runs.std(axis=0, ddof=1) / np.sqrt(8)
        dev = np.abs(mean - exact) / np.where(se > 0, se, 1.0)
        worst[name] = float(dev.max())
        print(f"{name}: worst deviation {dev.max():.2f} s.e. at beta = {ENUM_BETAS[dev.argmax()]:.1f}; s.e. at beta = 2: {se[-1]:.2e}")
        for k in range(ENUM_BETAS.size):
            assert abs(mean[k] - exact[k]) <= 4 * se[k] + 1e-12, (name, ENUM_BETAS[k], mean[k], exact[k], se[k])
    se_lnZ = np.array(lnZ).std(axis=0, ddof=1)[-1] / np.sqrt(8)
    miss = abs(np.array(lnZ_plain).mean(axis=0)[-1] - exact_lnZ[-1])
    print(f"control without resampling: ln Z at beta = 2 misses by {miss:.4f} = {miss / se_lnZ:.1f} s.e.")
    assert miss > 4 * se_lnZ, "the control agrees with the enumeration: the test has no power"


# ---------------------------------------------------------------- determinism and accounting
@pytest.mark.parametrize("shape,periodic", [((8, 24), True), ((2, 4, 20), (False, True, False))])
def test_determinism_split_runs_and_launch_count(hip, shape, periodic):
    R, theta, seed = 200, 3, 7
    dis = _disorder(shape, periodic, 8)
    betas = list(np.linspace(0.0, 1.0, 7))
    K = len(betas) - 1

    def fresh():
        return _handle(hip, shape, periodic, R, dis, betas, seed)
    a, b, c, d = fresh(), fresh(), fresh(), fresh()
    try:
        a.run(K, theta)
        ha = a.history()
        assert (ha["parent"] != np.arange(R)).any()
        assert a.launch_count() == 2 * theta * K and a.step_count == K and a.sweep_count == theta * K
        b.run(K, theta)
        hb = b.history()
        for key in ha:
            assert (ha[key] == hb[key]).all(), key  # the same seed twice
        c.run(K, theta, record=False)  # record=False leaves the same spins
        with pytest.raises(ValueError, match="recorded nothing"):
            c.history()
        assert (_planes(c) == _planes(a)).all()
        assert (c.energies()[0] == ha["E"][-1]).all()
        d.run(2, theta)  # a run split in two calls equals one call
        h1 = d.history()
        d.run(K - 2, theta)
        h2 = d.history()
        assert (h1["E"][-1] == h2["E"][0]).all()
        for key in ha:
            joined = np.concatenate([h1[key], h2[key][1:] if key in ("E", "M") else h2[key]])
            assert (joined == ha[key]).all(), key
        assert (_planes(d) == _planes(a)).all() and d.launch_count() == a.launch_count()
        with pytest.raises(ValueError, match="past the schedule"):
            d.run(1, theta)
    finally:
        for x in (a, b, c, d):
            x.close()


def test_model_layer_record_estimators_and_scan(hip):
    """PopulationAnnealing joins the records of split runs; free_energy, observables and family_stats are those of the record; the
    scan returns temperature_scan's keys plus ln_Z, rho_t, rho_s."""
    from tsu.models import ising
    betas = np.linspace(0.0, 1.0, 6)
    dis = _disorder((8, 8), True, 2, field=False)
    kw = dict(betas=betas, couplings=dis[:2], seed=3, sweeps_per_step=2)
    pa = ising.PopulationAnnealing(8, 300, **kw)
    pb = ising.PopulationAnnealing(8, 300, **kw)
    try:
        pa.run(2)
        h = pa.run()
        hb = pb.run()
        for key in hb:
            assert (h[key] == hb[key]).all(), key
        assert h["E"].shape == (6, 300) and h["parent"].shape == (5, 300) and h["resampled"].all()
        fe, ob, fam = pa.free_energy(), pa.observables(), pa.family_stats()
        want = ising.population_free_energy(betas, h["S"], h["E_min"], h["E"].mean(axis=1), 300, 64)
        for key in ("ln_Z", "F", "entropy"):
            np.testing.assert_array_equal(fe[key], want[key])
        assert fe["ln_Z"][0] == 64 * np.log(2.0) and (np.diff(fe["ln_Z"]) > 0).all()  # E_min < 0: Z grows with beta
        np.testing.assert_array_equal(ob["energy"], h["E"].mean(axis=1))
        np.testing.assert_array_equal(ob["abs_magnetization"], np.abs(h["M"] / 64.0).mean(axis=1))
        assert fam["families"][0] == 300 and (np.diff(fam["families"]) <= 0).all() and fam["rho_t"][0] == 1.0
        assert (fam["rho_t"] >= 1.0).all() and (fam["rho_s"] <= 300.0 + 1e-9).all()
        pc = ising.PopulationAnnealing(8, 300, **kw)
        pc.run(2, record=False)
        assert not pc.run(1, resample=False)["resampled"].any()  # a partial record says what its own run did
        part = pc.run()
        assert part["resampled"].all() and part["E"].shape == (3, 300)
        with pytest.raises(ValueError, match="every step"):
            pc.free_energy()
        pc._pa.close()
    finally:
        pa._pa.close()
        pb._pa.close()
    out = ising.population_annealing_scan(8, 300, **kw)
    for key in ("temperatures", "magnetization", "energy", "susceptibility", "specific_heat", "ln_Z", "rho_t", "rho_s"):
        assert np.shape(out[key]) == (6,), key
    np.testing.assert_array_equal(out["ln_Z"], fe["ln_Z"])
    np.testing.assert_allclose(out["energy"], ob["energy"] / 64, rtol=1e-14)  # the same record, summed by another NumPy call
    kf = dict(betas=betas, seed=3, sweeps_per_step=2)
    up = ising.population_annealing_scan(8, 300, external_field=0.5, **kf)
    same = ising.population_annealing_scan(8, 300, field=np.full((8, 8), 0.5), **kf)
    np.testing.assert_array_equal(up["ln_Z"], same["ln_Z"])
    assert (up["ln_Z"] != ising.population_annealing_scan(8, 300, **kf)["ln_Z"])[1:].all()
    out3 = ising.population_annealing_scan_3d((2, 4, 4), 100, temperatures=[np.inf, 4.0, 2.0], periodic=(False, True, True), seed=1,
                                              sweeps_per_step=1)
    assert out3["ln_Z"].shape == (3,) and out3["ln_Z"][0] == 32 * np.log(2.0) and np.isfinite(out3["specific_heat"]).all()


def test_other_handles_are_untouched_beside_a_population(hip):
    from tsu.models import ising
    dis = _disorder((8, 16), True, 4)
    Ts = [0.8, 1.6, 3.2]

    def others():
        one = ising.IsingModel2D((8, 16), temperature=1.1, seed=5, couplings=dis[:2], field=dis[2])
        one.gibbs_update(4)
        pt = ising.LatticeTempering((8, 16), Ts, couplings=dis[:2], field=dis[2], seed=6)
        h = pt.run(6, 2)
        out = (one.spins, one.energy(), h["E"].copy(), h["walker"].copy(), [pt.spins(w) for w in range(3)])
        pt._pt.close()
        return out
    want = others()
    pa = _handle(hip, (8, 16), True, 50, dis, [0.0, 0.5, 1.0], 5)
    try:
        pa.run(1, 2)
        got = others()
        pa.run(1, 2)
    finally:
        pa.close()
    assert (got[0] == want[0]).all() and got[1] == want[1] and (got[2] == want[2]).all() and (got[3] == want[3]).all()
    assert all((g == w).all() for g, w in zip(got[4], want[4]))


def test_errors(hip):
    z = np.zeros((4, 4), np.float32)
    for R in (1, 65536):
        with pytest.raises(ValueError, match="population must be in"):
            hip.PopulationLattice(4, 4, True, R)
        with pytest.raises(ValueError, match="population must be in"):
            hip.PopulationLattice3D(4, 4, 4, True, R)
    with pytest.raises(hip.UnsupportedError):
        hip.PopulationLattice(5, 4, True, 4)  # the lattice's own shape check
    pa = hip.PopulationLattice(4, 4, True, 4)
    try:
        for betas in ([0.5], [0.0, 0.0], [1.0, 0.5], [-1.0, 0.0], [0.0, float("inf")]):
            with pytest.raises(ValueError, match="set_schedule"):
                pa.set_schedule(betas)
        pa.set_schedule([0.0, 1.0])
        with pytest.raises(ValueError, match="set_disorder first"):
            pa.init(1)
        pa.set_disorder(z, z)
        for call in (lambda: pa.run(1, 1), pa.energies, lambda: pa.get_spins(0), lambda: pa.set_spins(0, z.astype(np.int8))):
            with pytest.raises(ValueError, match="init first"):
                call()
        pa.init(1)
        with pytest.raises(ValueError, match="past the schedule"):
            pa.run(2, 1)
        with pytest.raises(ValueError, match="sweeps_per_step"):
            pa.run(1, -1)
        with pytest.raises(ValueError, match="out of range"):
            pa.get_spins(4)
        pa.run(1, 1)
        assert pa.history()["E"].shape == (2, 4)
        pa.set_schedule([0.0, 1.0, 2.0])  # a new schedule asks for a new init
        with pytest.raises(ValueError, match="init first"):
            pa.run(1, 1)
    finally:
        pa.close()
    pb = hip.PopulationLattice(4, 4, True, 4)
    try:
        with pytest.raises(ValueError, match="set_disorder first"):
            pb.run(1, 1)
        pb.set_disorder(z, z)
        with pytest.raises(ValueError, match="set_schedule first"):
            pb.run(1, 1)
    finally:
        pb.close()

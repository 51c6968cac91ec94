"""K14 on the GPU (csrc/potts_pop.hip): populations of K12's Potts lattice.  Without resampling a walker is the single model and the
NumPy twin (tests/helpers/potts_pop_twin.py) on all three routes; resampled chains step by step against population_twin.check_step
and the twin's sweeps; the copy on planes whose stride is padded; 65535 walkers; the boundaries between the routes; split runs and
launch counts; equilibrium against full enumeration; the Python layer; and the refusals.  tests/test_potts_pop_cpu.py asserts that
the bit-for-bit cases hold no fragile decision."""
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


pp = _load("potts_pop_twin")
pdt, pop = pp.pdt, pp.pop
SWITCHES = {"k14_pop_pack": {}, "k14_pop_small": {"TSU_POTTS_POP_PACK": "0"}, "k14_pop_sweep": {"TSU_POTTS_SMALL": "0"}}


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    monkeypatch.delenv("TSU_POTTS_SMALL", raising=False)
    monkeypatch.delenv("TSU_POTTS_POP_PACK", raising=False)


def _set_route(monkeypatch, route):
    for name in ("TSU_POTTS_SMALL", "TSU_POTTS_POP_PACK"):
        monkeypatch.delenv(name, raising=False)
    for k, v in SWITCHES[route].items():
        monkeypatch.setenv(k, v)


def _population(shape, q, per, J, h, R, betas, seed, **kw):
    """The public class of the shape's dimension on the twin's disorder (its field is colour-major, the class takes shape + (q,))."""
    import tsu
    cls = tsu.PottsPopulationAnnealing if len(shape) == 2 else tsu.PottsPopulationAnnealing3D
    return cls(shape, q, R, betas=betas, couplings=J, site_field=None if h is None else np.moveaxis(h, 0, -1), periodic=per, seed=seed, **kw)


def _routes_of(shape, per, q, field, R):
    """The routes the switches can give this shape, the shipped one first."""
    first = pp.plan_of(shape, per, q, field, R)["route"]
    return [r for r in pp.ROUTES if pp.ROUTES.index(r) >= pp.ROUTES.index(first)]


_single_twins = {}


def _single_twin(c):
    """The twin's rows of a case, computed once and shared by the routes."""
    key = pp.case_id(c)
    if key not in _single_twins:
        tw = pp.single_twin(c)
        start = tw.spins.copy() if tw.betas[0] == 0 else None
        rows = tw.run(3, pp.SWEEPS_PER_STEP, resample=False)
        assert tw.fragile == 0
        _single_twins[key] = (tw, rows, start)
    return _single_twins[key]


@pytest.mark.parametrize("c", pp.single_cases(), ids=pp.case_id)
def test_without_resampling_a_walker_is_the_single_model_on_every_route(monkeypatch, c):
    """R = 70 walkers, three steps of two sweeps without resampling.  Walkers 0, G - 1, G and R - 1 (G of the shipped plan; the last
    group of 70 is partial on 6 x 32, 5 x 37 and 16 x 16, where G = 21, 17 and 16) equal PottsModel2D/3D(seed + i) swept at 1 / beta[k]
    from the walker's drawn colours, colours and energy bits, and equal the NumPy twin with n_eq and N; the draw equals the twin's for
    all walkers."""
    import tsu
    J, h = pp.case_disorder(c)
    sch = pp.SCHEDULES[c["schedule"]]
    betas, R, q, shape, per = sch["betas"], pp.R_SINGLE, c["q"], c["shape"], c["periodic"]
    tw, rows, _ = _single_twin(c)
    walkers = pp.single_walkers(c)
    one = tsu.PottsModel2D if len(shape) == 2 else tsu.PottsModel3D
    want_draw = pp.draw(shape, q, c["seed"], R)
    finals = []
    for route in _routes_of(shape, per, q, c["field"], R):
        _set_route(monkeypatch, route)
        # the draw alone, then the population proper (its init sweeps, when beta[0] > 0, follow the same draw)
        dev = _population(shape, q, per, J, h, R, [0.0, 1.0], c["seed"])
        try:
            assert all((dev.spins(i) == want_draw[i]).all() for i in range(R)), "the device draw differs from the twin's"
        finally:
            dev.close()
        dev = _population(shape, q, per, J, h, R, betas, c["seed"], sweeps_per_step=pp.SWEEPS_PER_STEP, initial_sweeps=sch["initial_sweeps"])
        try:
            assert dev.route() == route and dev.plan() == pp.plan_of(shape, per, q, c["field"], R, allow_pack=route == "k14_pop_pack",
                                                                     allow_small=route != "k14_pop_sweep")
            if c["sweep0"]:  # the counter's word wraps inside the run (init's own sweeps start from 0)
                dev._pa.advance(c["sweep0"])
            hist = dev.run(resample=False)
            assert (hist["parent"] == np.arange(R)).all() and not hist["W"].any() and not hist["S"].any() and not hist["E_min"].any()
            assert hist["E"][:, walkers].tobytes() == rows["E"].tobytes()
            assert (hist["n_eq"][:, walkers] == rows["n_eq"]).all() and (hist["N"][:, walkers] == rows["N"]).all()
            assert (hist["N"].sum(axis=2) == int(np.prod(shape))).all()
            for i in walkers:
                assert (dev.spins(i) == tw.spins[i]).all(), i
            # the single models: from the walker's colours before the first step
            s0 = sch["initial_sweeps"] if betas[0] > 0 else 0
            for i in walkers:
                m = one(shape, q, temperature=1.0 / betas[1] if betas[0] == 0 else 1.0 / betas[0], periodic=per, seed=(c["seed"] + i) % 2 ** 64,
                        couplings=J, site_field=None if h is None else np.moveaxis(h, 0, -1))
                try:
                    m.spins = want_draw[i]
                    if s0:
                        m.gibbs_update(s0)
                    m.sweep_count += c["sweep0"]
                    assert np.float64(m.energy()).tobytes() == np.float64(hist["E"][0, i]).tobytes()
                    for k in (1, 2, 3):
                        m.temperature = 1.0 / betas[k]
                        m.gibbs_update(pp.SWEEPS_PER_STEP)
                        assert np.float64(m.energy()).tobytes() == np.float64(hist["E"][k, i]).tobytes(), (i, k)
                    assert (m.spins == dev.spins(i)).all(), i
                finally:
                    m.close()
            # the draw, init's sweeps and pass, the identity rows of a record without resampling, three steps
            assert dev.launch_count() == 1 + pp.step_launches(route, s0, False) + 1 + 3 * pp.step_launches(route, pp.SWEEPS_PER_STEP, False)
            finals.append((np.stack([dev.spins(i) for i in range(R)]), hist["E"]))
        finally:
            dev.close()
    assert all((f[0] == finals[0][0]).all() and f[1].tobytes() == finals[0][1].tobytes() for f in finals[1:]), "the routes differ"


def _sample(R, parent):
    """The walkers whose planes are checked: all of a small population; else the ends, a stride and some of the dead."""
    if R <= 65:
        return list(range(R))
    dead = np.flatnonzero(np.asarray(parent) != np.arange(R))[:16].tolist()
    return sorted(set([0, 1, R // 2, R - 2, R - 1] + list(range(0, R, 41)) + dead))


@pytest.mark.parametrize("c", pp.CHAIN_CASES, ids=lambda c: "x".join(map(str, c["shape"])) + f"-q{c['q']}-R{c['R']}-db{c['db']}")
def test_resampled_chain_step_by_step(c):
    """Three resampled steps of two sweeps, one run per step.  W within one unit of NumPy's; S, U, E_min and parent recomputed from the
    device's E and W equal the device's; every checked plane is its parent's plane swept by the twin with the child's key; n_eq, N and
    E rows equal the twin's."""
    shape, q, per, R = c["shape"], c["q"], c["periodic"], c["R"]
    J, h = pdt.random_disorder(shape, per, q, np.random.default_rng(c["dseed"]), "gaussian", c["field"])
    betas = pp.chain_betas(c)
    dev = _population(shape, q, per, J, h, R, betas, c["seed"], sweeps_per_step=pp.CHAIN_SWEEPS, initial_sweeps=1)
    try:
        before = np.stack([dev.spins(i) for i in range(R)])
        start = pp.draw(shape, q, c["seed"], R)
        for i in _sample(R, np.arange(R)):
            assert (before[i] == pdt.sweep(start[i], q, per, J, h, 1.0 / betas[0], 1, c["seed"] + i, 0, 0)).all()
        moved = 0
        for j in range(pp.CHAIN_STEPS):
            rec = dev._pa.run(1, pp.CHAIN_SWEEPS, True, True) or dev._pa.history()
            parent = pop.check_step(rec["E"][0], rec["W"][0], betas[j + 1] - betas[j], j, c["seed"], rec["S"][0], rec["U"][0], rec["E_min"][0],
                                    rec["parent"][0])
            n = np.bincount(parent, minlength=R)
            assert n.sum() == R and (parent[n > 0] == np.flatnonzero(n > 0)).all()
            moved += int((n == 0).sum())
            after = np.stack([dev.spins(i) for i in range(R)])
            for i in _sample(R, parent):
                want, fragile = pdt.sweep(before[parent[i]], q, per, J, h, 1.0 / betas[j + 1], pp.CHAIN_SWEEPS, c["seed"] + i, 1 + pp.CHAIN_SWEEPS * j, 0,
                                          with_fragile=True)
                assert fragile == 0
                assert (after[i] == want).all(), (j, i)
                n_eq, N = pdt.measure(want, q, per)
                assert rec["n_eq"][1, i] == n_eq and (rec["N"][1, i] == N[:q]).all()
                assert np.float64(rec["E"][1, i]).tobytes() == np.float64(pdt.energy(want, q, per, J, h)).tobytes()
            before = after
        assert (moved > 0) == (c["db"] > 1e-6)
    finally:
        dev.close()


@pytest.mark.parametrize("shape,per", [((5, 37), False), ((3, 5, 18), (False, False, True))], ids=["5x37-o", "3x5x18-oop"])
def test_copy_on_awkward_planes(shape, per):
    """One step with a beta step of 5 and no sweeps: dead walkers hold their parents' colours, survivors are untouched, and the pad
    bytes between the walkers (185 -> 192, 270 -> 272 bytes) are zero before and after."""
    q, R, seed = 3, 40, 77
    J, h = pdt.random_disorder(shape, per, q, np.random.default_rng(3), "gaussian", True)
    dev = _population(shape, q, per, J, h, R, [0.0, 5.0], seed, sweeps_per_step=0)
    try:
        sites = int(np.prod(shape))
        assert pp.stride(sites) > sites
        before = np.stack([dev._pa.get_padded(i) for i in range(R)])
        assert not before[:, sites:].any() and (before[:, :sites].reshape((R,) + shape) == pp.draw(shape, q, seed, R)).all()
        hist = dev.run()
        parent = hist["parent"][0]
        n = np.bincount(parent, minlength=R)
        assert (n == 0).sum() > 5 and n.sum() == R
        after = np.stack([dev._pa.get_padded(i) for i in range(R)])
        assert (after == before[parent]).all() and not after[:, sites:].any()
        assert (after[n > 0] == before[n > 0]).all()
        assert hist["E"][1].tobytes() == hist["E"][0][parent].tobytes() and dev.launch_count() == 1 + 2 + 4
    finally:
        dev.close()


def test_largest_population_one_resampled_step():
    """R = 65535 at 4 x 4, q = 2: the record's shapes, check_step, sum n_i = R."""
    R, seed, betas = 65535, 2 ** 64 - 70000, [0.0, 0.4]
    J, h = pdt.random_disorder((4, 4), True, 2, np.random.default_rng(8), "gaussian", True)
    dev = _population((4, 4), 2, True, J, h, R, betas, seed, sweeps_per_step=1)
    try:
        hist = dev.run()
        assert hist["E"].shape == hist["n_eq"].shape == (2, R) and hist["N"].shape == (2, R, 2) and hist["W"].shape == hist["parent"].shape == (1, R)
        assert hist["S"].shape == hist["U"].shape == hist["E_min"].shape == (1,) and hist["W"].dtype == np.uint32 and hist["parent"].dtype == np.int32
        parent = pop.check_step(hist["E"][0], hist["W"][0], 0.4, 0, seed, hist["S"][0], hist["U"][0], hist["E_min"][0], hist["parent"][0])
        n = np.bincount(parent, minlength=R)
        assert n.sum() == R and (n == 0).any() and (parent[n > 0] == np.flatnonzero(n > 0)).all()
        for i in (0, 1, R - 1):
            assert (dev.spins(i) == pdt.sweep(pp.draw((4, 4), 2, seed + int(parent[i]), 1)[0], 2, True, J, h, 2.5, 1, (seed + i) % 2 ** 64, 0, 0)).all()
        assert (hist["N"].sum(axis=2) == 16).all() and dev.plan()["route"] == "k14_pop_pack"
    finally:
        dev.close()


BOUNDARY = [((128, 16), True, 3, False, "k14_pop_pack"),                     # 128 lanes a walker: the last shape whose walkers pair up
            ((130, 16), True, 3, False, "k14_pop_small"),                    # the next one past it
            ((2, 44, 16), (True, False, True), 8, True, "k14_pop_pack"),     # 64768 bytes of LDS: the last that fits 64 KiB
            ((2, 45, 16), (True, False, True), 8, True, "k14_pop_small"),    # 66240 bytes
            ((128, 128), True, 3, False, "k14_pop_small"),
            ((128, 130), True, 3, False, "k14_pop_sweep")]


@pytest.mark.parametrize("shape,per,q,field,route", BOUNDARY, ids=["x".join(map(str, b[0])) for b in BOUNDARY])
def test_route_boundaries(monkeypatch, shape, per, q, field, route):
    """Three walkers, two resampled steps of one sweep, on the shipped route and on every route the switches turn it into: the same
    record and the same colours; plan() equals the mirror."""
    J, h = pdt.random_disorder(shape, per, q, np.random.default_rng(12), "gaussian", field)
    results = []
    for r in _routes_of(shape, per, q, field, 3):
        _set_route(monkeypatch, r)
        dev = _population(shape, q, per, J, h, 3, [0.0, 0.3, 0.8], 91, sweeps_per_step=1)
        try:
            assert dev.route() == r and dev.plan() == pp.plan_of(shape, per, q, field, 3, allow_pack=r == "k14_pop_pack", allow_small=r != "k14_pop_sweep")
            hist = dev.run()
            results.append((hist, np.stack([dev.spins(i) for i in range(3)])))
        finally:
            dev.close()
    assert _routes_of(shape, per, q, field, 3)[0] == route
    hist, spins = results[0]
    assert np.float64(hist["E"][2, 1]).tobytes() == np.float64(pdt.energy(spins[1], q, per, J, h)).tobytes()
    for other, s in results[1:]:
        assert all(other[k].tobytes() == hist[k].tobytes() for k in hist) and (s == spins).all()


@pytest.mark.parametrize("shape,per", [((6, 32), True), ((130, 16), True)], ids=["6x32", "130x16"])
def test_split_run_equals_one_run_and_launch_counts(monkeypatch, shape, per):
    q, R, seed, betas, sps = 3, 23, 404, [0.1, 0.4, 0.8, 1.3, 1.9], 2
    J, h = pdt.random_disorder(shape, per, q, np.random.default_rng(14), "gaussian", True)
    for route in _routes_of(shape, per, q, True, R):
        _set_route(monkeypatch, route)
        runs = []
        for split in (None, None, 1):
            dev = _population(shape, q, per, J, h, R, betas, seed, sweeps_per_step=sps, initial_sweeps=2)
            try:
                base = dev.launch_count()
                assert base == 1 + pp.step_launches(route, 2, False)
                if split is None:
                    hist = dev.run()
                else:
                    dev.run(split)
                    assert dev.launch_count() == base + split * pp.step_launches(route, sps, True)
                    hist = dev.run()
                assert dev.launch_count() == base + 4 * pp.step_launches(route, sps, True)
                assert dev.step_count == 4 and dev.sweep_count == 2 + 4 * sps and hist["E"].shape == (5, R)
                E_now = dev.energies()
                assert E_now.tobytes() == hist["E"][-1].tobytes() and dev.launch_count() == base + 4 * pp.step_launches(route, sps, True) + 2
                runs.append((hist, np.stack([dev.spins(i) for i in range(R)])))
                with pytest.raises(ValueError):
                    dev.run(1)
            finally:
                dev.close()
        for hist, spins in runs[1:]:
            assert all(hist[k].tobytes() == runs[0][0][k].tobytes() for k in hist) and (spins == runs[0][1]).all()
        assert (runs[0][0]["parent"] != np.arange(R)).any()


@pytest.mark.parametrize("case", pp.ENUM_CASES, ids=lambda c: "x".join(map(str, c[0])) + f"-q{c[1]}")
def test_equilibrium_against_full_enumeration(case):
    """beta from 0 to 1.5 in 30 steps, 5 sweeps a step, M = 32 seeds of R = 1024 walkers: ln Z and <E> at every beta lie within 4
    standard errors (the spread over the M runs / sqrt(M)) of the sums over all q^N states.  The control, the same schedule without
    resampling and without sweeps, misses <E> at the last beta by more than that margin.  R = 1024, M = 32; worst observed ratio on an
    MI355X: 2.35 (3 x 4, q = 3) and 2.18 (2 x 2 x 3, q = 2); the plain NumPy reference at R = 256, M = 32 gives 3.40 and 3.18
    (tests/test_potts_pop_cpu.py), with other generators 2.4 - 3.1 at R = 256 and 2.0 at R = 1024."""
    shape, q, per, field, _ = case
    J, h = pp.enum_disorder(case)
    lnZ_x, E_x = pp.exact(pp.state_energies(shape, q, per, J, h), pp.ENUM_BETAS)
    lnZ, mE, ctl = [], [], []
    for m in range(pp.ENUM_M):
        dev = _population(shape, q, per, J, h, pp.ENUM_R, pp.ENUM_BETAS, 31000 + 5000 * m, sweeps_per_step=pp.ENUM_SWEEPS)
        try:
            hist = dev.run()
            fe = dev.free_energy()
            assert fe["ln_Z"][0] == int(np.prod(shape)) * np.log(float(q))
            lnZ.append(fe["ln_Z"])
            mE.append(hist["E"].mean(axis=1))
        finally:
            dev.close()
        dev = _population(shape, q, per, J, h, pp.ENUM_R, pp.ENUM_BETAS, 31000 + 5000 * m, sweeps_per_step=0)
        try:
            ctl.append(dev.run(resample=False)["E"][-1].mean())
        finally:
            dev.close()
    worst = pp.criterion(lnZ, mE, lnZ_x, E_x)
    print(f"{shape} q = {q}: worst |mean - exact| / error = {worst:.3f}")
    assert worst < pp.ENUM_SIGMAS
    ctl = np.array(ctl)
    assert abs(ctl.mean() - E_x[-1]) > pp.ENUM_SIGMAS * ctl.std(ddof=1) / math.sqrt(pp.ENUM_M)


def test_python_layer():
    import tsu
    shape, q, R, betas = (6, 18), 3, 48, np.linspace(0.0, 1.2, 5)
    J, h = pdt.random_disorder(shape, True, q, np.random.default_rng(2), "gaussian", True)
    pa = _population(shape, q, True, J, h, R, betas, 7, sweeps_per_step=2)
    try:
        hist = pa.run(2)
        hist = pa.run()
        want = {"E": (np.float64, (5, R)), "n_eq": (np.int64, (5, R)), "N": (np.int64, (5, R, q)), "W": (np.uint32, (4, R)), "parent": (np.int32, (4, R)),
                "S": (np.uint64, (4,)), "U": (np.uint64, (4,)), "E_min": (np.float64, (4,)), "resampled": (np.bool_, (4,))}
        assert sorted(hist) == sorted(want) and all(hist[k].dtype == d and hist[k].shape == s for k, (d, s) in want.items())
        fe = pa.free_energy()
        assert fe["ln_Z"][0] == 108 * np.log(3.0) and fe["ln_Z"].shape == (5,) and np.isnan(fe["F"][0]) and np.isfinite(fe["F"][1:]).all()
        assert np.allclose(fe["ln_Z"], pp.free_energy(list(betas), hist["S"], hist["E_min"], None, R, 108, q), rtol=0, atol=1e-9)
        assert np.allclose(fe["entropy"], betas * hist["E"].mean(axis=1) + fe["ln_Z"])
        ob = pa.observables()
        m = (q * hist["N"].max(axis=2) / 108.0 - 1.0) / (q - 1.0)
        assert np.allclose(ob["energy"], hist["E"].mean(axis=1)) and np.allclose(ob["energy_sq"], (hist["E"] ** 2).mean(axis=1))
        assert np.allclose(ob["equal_bonds"], hist["n_eq"].mean(axis=1)) and np.allclose(ob["order_parameter"], m.mean(axis=1))
        assert np.allclose(ob["order_parameter_sq"], (m ** 2).mean(axis=1))
        fam = pa.family_stats()
        assert fam["rho_t"][0] == 1.0 and fam["families"][0] == R and (np.diff(fam["families"]) <= 0).all() and fam["families"][-1] < R
        E = pa.energies()
        e, s = pa.best()
        i = int(E.argmin())
        assert e == E[i] and (s == pa.spins(i)).all() and e == E.min()
        assert np.float64(e).tobytes() == np.float64(pdt.energy(s, q, True, J, h)).tobytes()
        assert pa.route() == "k14_pop_pack" and pa.plan()["G"] == 21
    finally:
        pa.close()
    keys = {"energy", "order_parameter", "specific_heat", "susceptibility", "binder", "temperatures", "betas", "ln_Z", "F", "entropy", "rho_t", "rho_s"}
    out = tsu.potts_population_annealing_scan(shape, q, R, betas=betas, couplings=J, site_field=np.moveaxis(h, 0, -1), seed=7, sweeps_per_step=2)
    assert set(out) == keys and all(np.shape(out[k]) == (5,) for k in keys) and np.allclose(out["ln_Z"], fe["ln_Z"], rtol=0, atol=0)
    J3, h3 = pdt.random_disorder((2, 4, 18), True, 2, np.random.default_rng(2), "gaussian", False)
    out = tsu.potts_population_annealing_scan_3d((2, 4, 18), 2, 16, temperatures=[np.inf, 2.0, 1.0], couplings=J3, seed=7, sweeps_per_step=1)
    assert set(out) == keys and out["ln_Z"][0] == 144 * np.log(2.0) and out["temperatures"][0] == np.inf


def test_refusals_leave_nothing_behind():
    """The handle's refusals name what is wrong and change nothing; a K12 lattice and a K13 ladder beside a population give the same
    bits before and after."""
    import tsu
    from tsu import _hip
    shape, q = (6, 32), 3
    J, h = pdt.random_disorder(shape, True, q, np.random.default_rng(4), "gaussian", True)
    sf = np.moveaxis(h, 0, -1)

    def others():
        one = tsu.PottsModel2D(shape, q, temperature=0.9, seed=5, couplings=J, site_field=sf)
        lad = tsu.PottsTempering(shape, q, [0.7, 1.4], couplings=J, site_field=sf, seed=6)
        try:
            one.gibbs_update(3)
            hist = lad.run(2, 2)
            return one.spins.tobytes() + np.float64(one.energy()).tobytes() + b"".join(hist[k].tobytes() for k in sorted(hist))
        finally:
            one.close()
            lad.close()
    ref = others()
    pa = _hip.PottsPopulation(shape, q, True, 10)
    try:
        with pytest.raises(ValueError, match="call tsu_potts_pop_set_disorder first"):
            pa.init(1)
        pa.set_disorder(J[0], J[1], None, h)
        with pytest.raises(ValueError, match="call tsu_potts_pop_set_schedule first"):
            pa.init(1)
        with pytest.raises(ValueError, match="call tsu_potts_pop_set_schedule first"):
            pa.run(1, 1)
        for bad, msg in (([0.5], "need 2 to"), ([0.5, 0.5], "betas must increase"), ([-1.0, 0.5], "beta\\[0\\] must be finite and >= 0")):
            with pytest.raises(ValueError, match=msg):
                pa.set_schedule(bad)
        pa.set_schedule([0.0, 0.5, 1.0])
        with pytest.raises(ValueError, match="call tsu_potts_pop_init first"):
            pa.run(1, 1)
        with pytest.raises(ValueError, match="call tsu_potts_pop_init first"):
            pa.energies()
        with pytest.raises(ValueError, match="initial must be"):
            pa.init(1, 3)
        with pytest.raises(ValueError, match="open axis|non-finite"):
            pa.set_disorder(np.full(shape, np.nan, np.float32), J[1], None, h)
        pa.init(1)
        with pytest.raises(ValueError, match="run past the schedule"):
            pa.run(3, 1)
        with pytest.raises(ValueError, match="out of range"):
            pa.get_spins(10)
        with pytest.raises(ValueError, match="outside 0 .. 2"):
            pa.set_spins(0, np.full(shape, 3, np.int8))
        with pytest.raises(ValueError, match="recorded nothing"):
            pa.history()
        before = np.stack([pa.get_spins(i) for i in range(10)])
        assert (before == pp.draw(shape, q, 1, 10)).all()
        pa.run(2, 1)
        assert others() == ref
        pa.set_schedule([0.0, 1.0])
        with pytest.raises(ValueError, match="call tsu_potts_pop_init first"):
            pa.run(1, 1)
    finally:
        pa.close()
    for kw, msg in ((dict(population=1), "population must be in"), (dict(population=65536), "population must be in"), (dict(q=9), "q must be in 2 .. 8"),
                    (dict(shape=(5, 32)), "periodic axis needs an even length")):
        args = dict(shape=shape, q=q, periodic=True, population=10)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            _hip.PottsPopulation(**args)
    assert others() == ref

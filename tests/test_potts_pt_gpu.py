"""K13 on the GPU (csrc/potts_pt.hip): tempering ladders of K12's Potts lattice bit for bit against the NumPy twin
(tests/helpers/potts_pt_twin.py) on both routes -- history, contingency tables, swap statistics, final colours and launch counts --,
walkers without swaps against the single models, split runs, a ladder of 130 temperatures, the boundary between the two routes, the
enumeration case of the CPU file on the device, and the refusals.  Every bit-for-bit case first asserts on the CPU that its inputs hold
no fragile decision (the twin's docstring says what that is)."""
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


pt = _load("potts_pt_twin")
pdt = pt.pdt


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    monkeypatch.delenv("TSU_POTTS_SMALL", raising=False)


def _ladder(c, J, h, T=None, **kw):
    """The public class of the case's dimension on the twin's disorder (its field is colour-major, the class takes shape + (q,))."""
    import tsu
    cls = tsu.PottsTempering if len(c["shape"]) == 2 else tsu.PottsTempering3D
    lad = cls(c["shape"], c["q"], pt.case_temperatures(c["R"]) if T is None else T, couplings=J,
              site_field=None if h is None else np.moveaxis(h, 0, -1), periodic=c["periodic"], seed=c["seed"], ladders=c["ladders"], **kw)
    if c.get("sweep0"):
        lad._pt.advance(c["sweep0"])
    return lad


def _energies_by_walker(hist):
    """energies(j, k) for the twin from the device's record: E by walker of ladder k in round j."""
    E, W = hist["E"], hist["walker"]

    def energies(j, k):
        out = np.empty(E.shape[2])
        out[W[j, k]] = E[j, k]
        return out
    return energies


def _assert_equals_twin(dev, twin, hist, want):
    assert hist["E"].tobytes() == want["E"].tobytes()
    for key in ("n_eq", "N", "walker"):
        assert (hist[key] == want[key]).all(), key
    if twin.nl == 2:
        assert (hist["tables"] == want["tables"]).all() and (hist["tables"].sum(axis=(2, 3)) == int(np.prod(twin.shape))).all()
        assert (hist["overlap"] == pt.overlap(want["tables"], twin.q)).all()
    else:
        assert "tables" not in hist
    st = dev.stats()
    assert (st["attempts"] == twin.attempts).all() and (st["accepts"] == twin.accepts).all()
    assert (st["round_trips"] == twin.trips).all() and (st["walker_at_slot"] == twin.walker_at_slot).all()
    assert st["sweep_count"] == twin.sweeps and st["round_count"] == twin.rounds
    assert dev.launch_count() == twin.launches
    for k in range(twin.nl):
        for i in range(twin.R):
            assert (dev.spins(k, i) == twin.spins[k][twin.walker_at_slot[k, i]]).all(), (k, i)
    # the energies now are the twin's ordered sums of the same colours, bit for bit
    assert dev.energies().tobytes() == twin.energies().tobytes()


@pytest.mark.parametrize("case", pt.cases(), ids=pt.case_id)
def test_ladder_equals_the_twin_on_both_routes(monkeypatch, case):
    """4 rounds of 3 sweeps with swaps: everything the handle reports, on k13_pt_small and, with TSU_POTTS_SMALL=0, on k13_pt_sweep."""
    J, h = pt.case_disorder(case)
    check = pt.case_twin(case)
    check_rows = check.run(pt.N_ROUNDS, pt.INTERVAL)
    assert check.fragile == 0
    for route in ("k13_pt_small", "k13_pt_sweep"):
        if route == "k13_pt_sweep":
            monkeypatch.setenv("TSU_POTTS_SMALL", "0")
        dev = _ladder(case, J, h)
        try:
            assert dev.route() == route
            hist = dev.run(pt.N_ROUNDS, pt.INTERVAL)
            twin = pt.case_twin(case, small=route == "k13_pt_small")
            want = twin.run(pt.N_ROUNDS, pt.INTERVAL, energies=_energies_by_walker(dev._pt.history()))
            assert twin.fragile == 0 and twin.attempts.sum() > 0
            _assert_equals_twin(dev, twin, hist, want)
            # the device's energies are the ones the twin sums by itself, so the CPU run above made the same swaps
            assert want["E"].tobytes() == check_rows["E"].tobytes() and (twin.walker_at_slot == check.walker_at_slot).all()
        finally:
            dev.close()


@pytest.mark.parametrize("shape,per", [((6, 32), True), ((3, 4, 18), (False, True, True))], ids=["6x32-p", "3x4x18-opp"])
def test_without_swaps_a_walker_is_the_single_model(monkeypatch, shape, per):
    import tsu
    q, T, seed = 3, [0.7, 1.1, 1.9], 4321
    J, h = pdt.random_disorder(shape, per, q, np.random.default_rng(5), "gaussian", True)
    site_field = np.moveaxis(h, 0, -1)
    cls, one = (tsu.PottsTempering, tsu.PottsModel2D) if len(shape) == 2 else (tsu.PottsTempering3D, tsu.PottsModel3D)
    for small in (True, False):
        if not small:
            monkeypatch.setenv("TSU_POTTS_SMALL", "0")
        dev = cls(shape, q, T, couplings=J, site_field=site_field, periodic=per, seed=seed, ladders=2)
        try:
            assert dev.run(2, 2, swap=False, record=False) is None
            assert (dev.walker_at_slot == np.arange(3)).all() and dev.launch_count() == (2 if small else 8)
            E = dev.energies()
            for g in range(6):
                m = one(shape, q, temperature=T[g % 3], periodic=per, seed=seed + g, couplings=J, site_field=site_field)
                try:
                    m.gibbs_update(4)
                    assert (dev.spins(g // 3, g % 3) == m.spins).all(), g
                    assert np.float64(E[g // 3, g % 3]).tobytes() == np.float64(m.energy()).tobytes(), g
                finally:
                    m.close()
        finally:
            dev.close()


def test_a_run_split_in_two_equals_one_run(monkeypatch):
    case = dict(shape=(5, 19), periodic=False, q=3, field=True, R=5, ladders=2, seed=99, dseed=370, sweep0=0)
    J, h = pt.case_disorder(case)
    for small in (True, False):
        if not small:
            monkeypatch.setenv("TSU_POTTS_SMALL", "0")
        a, b = _ladder(case, J, h), _ladder(case, J, h)
        try:
            whole = a.run(4, 3)
            first = b.run(1, 3)
            rest = b.run(3, 3)
            for key in ("E", "n_eq", "N", "walker", "tables"):
                assert np.concatenate([first[key], rest[key]]).tobytes() == whole[key].tobytes(), key
            sa, sb = a.stats(), b.stats()
            assert all(np.array_equal(sa[k], sb[k]) for k in sa) and sa["accepts"].sum() > 0
            assert all((a.spins(k, i) == b.spins(k, i)).all() for k in range(2) for i in range(5))
            assert a.launch_count() == b.launch_count()
        finally:
            a.close()
            b.close()


def test_long_ladder_of_130_temperatures():
    """R = 130, two ladders: more than one 64-lane pass over the swap kernel's tables, and the [ladder][slot] strides of the record."""
    c = pt.LONG
    J, h = pt.case_disorder(c)
    dev = _ladder(c, J, h)
    try:
        hist = dev.run(pt.LONG_ROUNDS, pt.LONG_INTERVAL)
        twin = pt.case_twin(c)
        want = twin.run(pt.LONG_ROUNDS, pt.LONG_INTERVAL, energies=_energies_by_walker(dev._pt.history()))
        assert twin.fragile == 0 and 0 < twin.accepts.sum() < twin.attempts.sum()
        _assert_equals_twin(dev, twin, hist, want)
    finally:
        dev.close()


@pytest.mark.parametrize("case", pt.BOUNDARY, ids=["128x128", "128x130"])
def test_route_boundary(case):
    """16384 sites are k13_pt_small's last lattice, 16640 k13_pt_sweep's first (128 x 130: the scalar path, more than one workgroup)."""
    J, h = pt.case_disorder(case)
    dev = _ladder(case, J, h)
    try:
        assert dev.route() == ("k13_pt_small" if case["shape"] == (128, 128) else "k13_pt_sweep")
        hist = dev.run(1, 1)
        twin = pt.case_twin(case)
        want = twin.run(1, 1, energies=_energies_by_walker(dev._pt.history()))
        assert twin.fragile == 0
        _assert_equals_twin(dev, twin, hist, want)
    finally:
        dev.close()


def test_equilibrium_on_the_device_against_enumeration():
    """The CPU file's case through PottsTempering.run in one call: open 3 x 4, q = 3 glass with a site field, T = 0.5 .. 2, 20 500
    rounds of one sweep from colour 0, the first 500 discarded; <E> at every slot within 4 batch-means errors of the enumeration."""
    import tsu
    E = pt.ENUM
    J, h = pt.enum_disorder()
    exact = pt.exact_energies(E["shape"], E["q"], E["periodic"], J, h, E["T"])
    dev = tsu.PottsTempering(E["shape"], E["q"], E["T"], couplings=J, site_field=np.moveaxis(h, 0, -1), periodic=E["periodic"], seed=E["seed"],
                             initial=0)
    try:
        assert dev.route() == "k13_pt_small"
        hist = dev.run(E["n_rounds"], 1)
        assert dev.launch_count() == 5 * E["n_rounds"]
        out = hist["E"][E["n_discard"]:, 0]
        err = np.array([pt.batch_means_error(out[:, i]) for i in range(len(E["T"]))])
        dev_err = (out.mean(axis=0) - exact) / err
        st = dev.stats()
        print(f"\n<E> = {out.mean(axis=0)}, exact = {exact}, error = {err}, (E - exact) / error = {dev_err}, "
              f"acceptance = {dev.swap_acceptance}, round trips = {st['round_trips']}")
        assert (np.abs(dev_err) <= 4.0).all()
        assert (st["attempts"] == E["n_rounds"]).all() and dev.round_trips > 0
    finally:
        dev.close()


def test_scan_reports_the_ladder(monkeypatch):
    """potts_tempering_scan's keys from a short two-replica ladder: the energy of the record, overlaps in [-1 / (q - 1), 1]."""
    from tsu.models import potts_tempering
    J, h = pdt.random_disorder((6, 6), True, 3, np.random.default_rng(8), "gaussian", False)
    T = [0.8, 1.2, 1.8]
    out = potts_tempering.potts_tempering_scan((6, 6), 3, T, n_equilibrate=20, n_measure=30, measure_every=2, seed=12, couplings=J, replicas=2)
    assert set(out) == {"energy", "order_parameter", "specific_heat", "susceptibility", "binder", "temperatures", "swap_acceptance",
                        "round_trips", "overlap", "overlap_sq", "overlap_binder"}
    assert all(np.shape(out[k]) == (3,) for k in out if k not in ("swap_acceptance", "round_trips")) and out["swap_acceptance"].shape == (2,)
    assert (out["overlap"] >= -0.5).all() and (out["overlap"] <= 1.0).all() and (out["overlap_sq"] >= out["overlap"] ** 2 - 1e-15).all()
    lad = potts_tempering.PottsTempering((6, 6), 3, T, couplings=J, seed=12, ladders=2)
    try:
        lad.run(10, 2, record=False)
        hist = lad.run(30, 2)
        assert (out["energy"] == (hist["E"][:, 0].T / 36).mean(axis=1)).all()
        assert (out["overlap"] == hist["overlap"].T.mean(axis=1)).all()
    finally:
        lad.close()


def test_refusals_leave_nothing_behind():
    from tsu import _hip
    ok = dict(shape=(4, 6), q=3, periodic=True, n_temps=3, n_ladders=1)

    def create(**kw):
        args = dict(ok)
        args.update(kw)
        return _hip.PottsTemperingLattice(**args)
    for kw in (dict(n_temps=1), dict(n_temps=257), dict(n_ladders=3), dict(n_ladders=0), dict(shape=(3, 6)), dict(shape=(4, 5)), dict(q=9), dict(q=1),
               dict(shape=(2, 3, 6), periodic=(True, True, True)), dict(shape=(0, 6), periodic=False)):
        with pytest.raises(ValueError):
            create(**kw)
    # never created: the next handle works as if nothing had happened
    J = pdt.constant_couplings((4, 6), True, 1.0)
    lat = create()
    try:
        with pytest.raises(ValueError, match="set_disorder first"):
            lat.run(1, 1)
        lat.set_disorder(*J)
        with pytest.raises(ValueError, match="set_temperatures first"):
            lat.run(1, 1)
        for bad in ([1.0, 0.0, 2.0], [1.0, -1.0, 2.0], [1.0, float("nan"), 2.0], [1.0, 2.0, float("inf")]):
            with pytest.raises(ValueError, match="Temperature must be positive"):
                lat.set_temperatures(bad)
        with pytest.raises(ValueError, match="set_temperatures first"):  # a refused ladder of temperatures was not stored
            lat.run(1, 1)
        lat.set_temperatures([1.0, 1.5, 2.0])
        with pytest.raises(ValueError, match="init first"):
            lat.run(1, 1)
        with pytest.raises(ValueError):
            lat.init(5, 3)
        lat.init(5, 1)
        for args in ((-1, 1), (1, 0)):
            with pytest.raises(ValueError):
                lat.run(*args)
        with pytest.raises(ValueError):
            lat.set_spins(0, 0, np.full((4, 6), 3, np.int8))
        for where in ((1, 0), (0, 3), (-1, 0)):
            with pytest.raises(ValueError):
                lat.get_spins(*where)
        nan = J[0].copy()
        nan[1, 2] = float("nan")
        with pytest.raises(ValueError, match="non-finite"):
            lat.set_disorder(nan, J[1])
        assert lat.launch_count() == 0 and (lat.get_spins(0, 2) == 1).all() and lat.stats()["sweep_count"] == 0
        # the handle is still usable, and on the disorder and temperatures it had
        lat.run(2, 2)
        twin = pt.Ladders((4, 6), 3, True, J, None, [1.0, 1.5, 2.0], 5, 1, initial=1)
        want = twin.run(2, 2)
        assert twin.fragile == 0 and lat.history()["E"].tobytes() == want["E"].tobytes() and (lat.history()["walker"] == want["walker"]).all()
        assert all((lat.get_spins(0, i) == twin.spins[0][twin.walker_at_slot[0, i]]).all() for i in range(3))
    finally:
        lat.close()
    # an open axis's last slice must be 0; one ladder has no tables
    lat = create(shape=(3, 5), periodic=False)
    try:
        with pytest.raises(ValueError, match="last column"):
            lat.set_disorder(np.ones((3, 5), np.float32), np.zeros((3, 5), np.float32))
        jd = np.ones((3, 5), np.float32)
        with pytest.raises(ValueError, match="last row"):
            lat.set_disorder(np.zeros((3, 5), np.float32), jd)
        with pytest.raises(ValueError, match="two ladders"):
            lat.ctx.check(lat.lib.tsu_potts_pt_overlap_tables(lat.h, None))
        with pytest.raises(ValueError, match="set_disorder first"):
            lat.run(1, 1)
    finally:
        lat.close()
    lat = create(shape=(2, 3, 5), periodic=(False, False, False))
    try:
        J3 = [np.zeros((2, 3, 5), np.float32) for _ in range(3)]
        with pytest.raises(ValueError, match="needs J_layer"):
            lat.set_disorder(J3[0], J3[1])
        J3[2][1, 0, 0] = 1.0
        with pytest.raises(ValueError, match="last layer"):
            lat.set_disorder(*J3)
    finally:
        lat.close()

"""K11 on the GPU (csrc/potts_muca.hip): the multicanonical walkers bit for bit against the NumPy twin
(tests/helpers/potts_muca_twin.py) -- spins, n_eq, H, S1, S2 and tunnel events -- on every route, on both sides of every size
switch and with every tail of a wave and of a workgroup; the handle's refusals and its consistency check; exact sampling of
arbitrary weights on the device; and canonical weights against K10's heat bath."""
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


mt = _load("potts_muca_twin")
ROUTES = ("k11_muca_lds", "k11_muca_global", "k11_muca_atomics")
FULL_SEED = 2 ** 64 - 59


@pytest.fixture(scope="module")
def hip():
    from tsu import _hip
    return _hip


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in ("TSU_POTTS_MUCA_ROUTE", "TSU_POTTS_MUCA_BLOCK"):
        monkeypatch.delenv(name, raising=False)


def _weights(B, kind, rng):
    """ln W with tied and steep entries: 'mixed' has both next to ordinary ones, 'canonical' is n / T."""
    if kind == "canonical":
        return np.arange(B + 1) / 1.3
    lnw = 0.15 * np.arange(B + 1) + rng.normal(size=B + 1)
    if B >= 6:
        lnw[1::5] = lnw[0]       # ties: thr = 2^32 both ways
        lnw[B // 2] = -45.0      # a drop no uniform passes: thr = 0
        lnw[B - 1] = lnw[B]
    return lnw


def _start(kind, W, shape, q, rng):
    if kind == "random":
        return rng.integers(0, q, size=(W,) + shape).astype(np.int8)
    return np.full((W,) + shape, int(kind), np.int8)  # every walker at n = B


def _compare(h, want, where):
    got = h.get_spins()
    assert (got == want["spins"]).all(), (where, "spins", int(np.count_nonzero(got != want["spins"])))
    assert (h.energies() == want["n"]).all(), (where, "n_eq")
    H, S1, S2 = h.record()
    assert (H == want["H"]).all() and (S1 == want["S1"]).all() and (S2 == want["S2"]).all(), (where, "record")
    assert (h.tunnels() == want["tunnels"]).all(), (where, "tunnels")
    assert h.measure(), (where, "the incremental n_eq / N_c differ from a recount")


def _run_case(hip, shape, per, q, W, start_kind, weight_kind, n_sweeps=4, seed=FULL_SEED, sweep0=2 ** 32 - 3, replica=3, routes=None,
              rng_seed=0):
    rng = np.random.default_rng(rng_seed)
    B, zmax = mt.geometry(shape, per)
    lnw = _weights(B, weight_kind, rng)
    start = _start(start_kind, W, shape, q, rng)
    bounds = (B // 3, B - B // 3) if B >= 3 else (0, max(B, 1))
    want = mt.run(start, q, per, lnw, n_sweeps, seed, sweep0, replica, bounds=bounds)
    h = hip.PottsMucaWalkers(*shape, q, W, per)
    assert (h.bonds, h.z_max) == (B, zmax)
    auto = ROUTES.index(h.route())
    for r in (range(auto, 3) if routes is None else routes):
        os.environ["TSU_POTTS_MUCA_ROUTE"] = str(r)
        try:
            assert h.route() == ROUTES[max(r, auto)]
            h.set_weights(lnw)
            if start_kind == "random":
                h.set_spins(start)
            else:
                h.fill(int(start_kind))
            h.set_tunnel_bounds(*bounds)
            h.clear_record()
            before = h.launch_count()
            h.run(n_sweeps, seed, sweep0, replica)
            assert h.launch_count() == before + 1
            _compare(h, want, (shape, per, q, W, ROUTES[max(r, auto)]))
        finally:
            del os.environ["TSU_POTTS_MUCA_ROUTE"]
    h.close()
    return want


# (shape, periodic, q, walkers, start, weights): odd site counts (the last site has no block partner), double bonds, odd periodic
# sides, a periodic axis of length 1, 3-D with mixed flags, q = 2 and q = 8, starts at n = B and random, tails of a wave
OPEN2, PER2 = (False, False, False), (False, True, True)
CASES = [((1, 3, 3), OPEN2, 3, 65, "random", "mixed"),
         ((1, 1, 7), OPEN2, 2, 3, "random", "mixed"),
         ((1, 5, 1), OPEN2, 5, 130, 1, "mixed"),
         ((1, 2, 2), PER2, 4, 257, "random", "mixed"),
         ((1, 2, 6), PER2, 8, 65, 7, "mixed"),
         ((1, 3, 5), PER2, 3, 130, "random", "mixed"),
         ((1, 1, 6), PER2, 3, 1, "random", "mixed"),
         ((1, 5, 1), PER2, 2, 257, 0, "canonical"),
         ((2, 3, 4), (True, False, True), 3, 130, "random", "mixed"),
         ((2, 3, 4), (True, False, True), 8, 3, 2, "canonical"),
         ((2, 2, 2), (True, True, True), 2, 65, "random", "mixed"),
         ((1, 1, 1), (True, True, True), 3, 65, "random", "mixed")]


def _case_id(c):
    return "x".join(map(str, c[0])) + "-" + "".join("p" if x else "o" for x in c[1]) + f"-q{c[2]}-w{c[3]}-{c[4]}-{c[5]}"


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_device_equals_the_twin_on_every_route(hip, case):
    """4 sweeps with a full-width seed, sweep0 = 2^32 - 3 (across the wrap) and replica 3, on all three routes."""
    shape, per, q, W, start, weights = case
    _run_case(hip, shape, per, q, W, start, weights, rng_seed=sum(shape) * 100 + q)


@pytest.mark.parametrize("walkers", [1, 3, 65, 130, 257])
@pytest.mark.parametrize("block", [None, 64, 128])
def test_tails_of_a_wave_and_of_a_workgroup(hip, monkeypatch, walkers, block):
    """The same walkers whatever the workgroup size: 65 = one wave and one lane, 130 = one 128-thread workgroup and two lanes."""
    if block is not None:
        monkeypatch.setenv("TSU_POTTS_MUCA_BLOCK", str(block))
    _run_case(hip, (1, 4, 5), PER2, 4, walkers, "random", "mixed", n_sweeps=3, rng_seed=9)


def test_a_split_run_equals_one_run(hip):
    """6 sweeps in one call against 2 + 4 with sweep0 advanced across the 32-bit wrap, records and tunnel state accumulated; every
    route."""
    shape, per, q, W = (1, 4, 6), PER2, 3, 130
    rng = np.random.default_rng(4)
    B, _ = mt.geometry(shape, per)
    lnw = _weights(B, "mixed", rng)
    start = _start("random", W, shape, q, rng)
    bounds = (B // 3, B - B // 3)
    sweep0 = 2 ** 32 - 1
    want = mt.run(start, q, per, lnw, 6, FULL_SEED, sweep0, 2, bounds=bounds)
    for r in range(3):
        os.environ["TSU_POTTS_MUCA_ROUTE"] = str(r)
        try:
            h = hip.PottsMucaWalkers(*shape, q, W, per)
            h.set_weights(lnw)
            h.set_spins(start)
            h.set_tunnel_bounds(*bounds)
            h.run(2, FULL_SEED, sweep0, 2)
            assert h.measure()
            h.run(4, FULL_SEED, (sweep0 + 2) & 0xFFFFFFFF, 2)
            assert h.launch_count() == 2
            _compare(h, want, ("split", ROUTES[r]))
            # a different replica or seed is a different stream
            h.set_spins(start)
            h.run(6, FULL_SEED, sweep0, 1)
            assert (h.get_spins() != want["spins"]).any()
            h.close()
        finally:
            del os.environ["TSU_POTTS_MUCA_ROUTE"]


# both sides of the two size switches (LDS cap 160 KiB: 62 (B + 1) bytes of histogram and table, plus 64 lattices for the LDS route)
@pytest.mark.parametrize("rows,cols,route", [(29, 29, "k11_muca_lds"), (30, 30, "k11_muca_global"), (36, 37, "k11_muca_global"),
                                             (37, 37, "k11_muca_atomics")])
def test_both_sides_of_every_size_switch(hip, rows, cols, route):
    shape = (1, rows, cols)
    h = hip.PottsMucaWalkers(*shape, 3, 64, OPEN2)
    assert h.route() == route
    h.close()
    _run_case(hip, shape, OPEN2, 3, 70, "random", "mixed", n_sweeps=2, routes=(0,), rng_seed=rows)


def test_a_lattice_beyond_the_lds_histogram(hip):
    """96 x 96, 64 walkers, 2 sweeps: 3 (B + 1) words far exceed the LDS, so the record takes global atomics and the table L2."""
    _run_case(hip, (1, 96, 96), PER2, 8, 64, "random", "canonical", n_sweeps=2, routes=(0,), rng_seed=96)


def test_handle_checks(hip):
    shape, per, q, W = (1, 3, 4), OPEN2, 3, 10
    h = hip.PottsMucaWalkers(*shape, q, W, per)
    B = h.bonds
    assert (h.get_spins() == 0).all() and (h.energies() == B).all() and h.measure() and h.launch_count() == 0
    rng = np.random.default_rng(0)
    s = rng.integers(0, q, size=(W,) + shape).astype(np.int8)
    h.set_spins(s)
    n, _ = mt.count(s, q, per)
    assert (h.energies() == n).all()
    for bad_value in (q, -1):
        bad = s.copy()
        bad[W - 1, 0, 2, 3] = bad_value
        with pytest.raises(Exception, match="outside 0"):
            h.set_spins(bad)
        assert (h.get_spins() == s).all() and (h.energies() == n).all()
    for length in (B, B + 2):
        with pytest.raises(Exception, match="weights for B"):
            h.set_weights(np.zeros(length))
    with pytest.raises(Exception, match="not finite"):
        h.set_weights(np.r_[np.zeros(B), np.nan])
    with pytest.raises(Exception, match="colour"):
        h.fill(q)
    for lo, hi in ((-1, 3), (3, 3), (2, B + 1)):
        with pytest.raises(Exception, match="n_lo"):
            h.set_tunnel_bounds(lo, hi)
    with pytest.raises(ValueError):
        h.run(1, 1, 0, 2 ** 24)
    assert (h.get_spins() == s).all() and h.launch_count() == 0
    h.run(0, 1)
    assert h.launch_count() == 0 and int(h.record()[0].sum()) == 0
    for k in range(3):
        h.run(2, 5, 2 * k)
        assert h.measure() and h.launch_count() == k + 1
    assert int(h.record()[0].sum()) == 6 * W
    h.clear_record()
    assert all(int(a.sum()) == 0 for a in h.record())
    h.close()
    for kw in (dict(q=1), dict(q=9), dict(walkers=0), dict(walkers=2 ** 20 + 1), dict(rows=0), dict(rows=300, cols=300),
               dict(rows=256, cols=256, walkers=2 ** 15)):
        a = dict(depth=1, rows=4, cols=4, q=3, walkers=8)
        a.update(kw)
        with pytest.raises(Exception):
            hip.PottsMucaWalkers(a["depth"], a["rows"], a["cols"], a["q"], a["walkers"], False)


def test_the_python_class_follows_the_twin_through_the_recursion():
    """Three iterations of the class against the twin's histograms and the package's recursion, then the record's by-products."""
    import tsu
    from tsu.models import potts_muca as pm
    shape, q, W, seed = (3, 5), 3, 200, 77
    m = tsu.PottsMulticanonical(shape, q, W, periodic=True, seed=seed)
    assert m.route() == "k11_muca_lds" and m.bonds == 30 and m.spins.shape == (W, 3, 5)
    m.set_tunnel_bounds(10, 24)
    s = np.zeros((W, 1, 3, 5), np.int8)
    lnw = np.zeros(31)
    side, tun, t = None, None, 0
    for it in range(3):
        info = m.iterate(10)
        out = mt.run(s, q, (False, True, True), lnw, 10, seed, sweep0=t, side=side, tunnels=tun, bounds=(10, 24))
        events = int(out["tunnels"].sum()) - (0 if tun is None else int(tun.sum()))
        s, side, tun, t = out["spins"], out["side"], out["tunnels"], t + 10
        lo, hi, flat, holes = pm.muca_flatness(out["H"])
        assert info["range"] == (lo, hi) and info["flatness"] == flat and info["holes"] == holes and info["tunnel_events"] == events
        assert (m.histogram() == out["H"]).all() and m.consistent()
        lnw = pm.muca_recursion(lnw, out["H"])
        assert m.weights.tobytes() == lnw.tobytes()
    assert (m.spins.reshape(s.shape) == s).all() and m.launch_count() == 3 and m.sweep_count == 30
    m.clear_record().run(5)
    out = mt.run(s, q, (False, True, True), lnw, 5, seed, sweep0=t, side=side, tunnels=tun, bounds=(10, 24))
    s1, s2 = m.moments()
    assert (s1 == out["S1"]).all() and (s2 == out["S2"]).all() and (m.tunnels() == out["tunnels"]).all()
    assert m.density_of_states().tobytes() == pm.muca_density_of_states(out["H"], lnw, q, 15).tobytes()
    r = m.reweight([0.8, 2.0])
    w = pm.muca_reweight(out["H"], out["S1"], out["S2"], lnw, [0.8, 2.0], 1.0, q, 15)
    assert all(r[k].tobytes() == w[k].tobytes() for k in w)
    m.close()
    res = tsu.potts_multicanonical_scan((2, 4), 4, [0.9, 1.5], walkers=512, n_iterations=4, sweeps_per_iteration=10, n_production=20,
                                        periodic=(False, True), seed=3)
    assert res["ln_g"].shape == (13,) and len(res["iterations"]) == 4 and res["tunnel_events"].shape == (512,)
    assert abs(np.exp(res["ln_g"][np.isfinite(res["ln_g"])]).sum() - 4.0 ** 8) < 1e-3 and res["energy"][0] < res["energy"][1] < 0


def test_device_samples_arbitrary_weights_exactly():
    """The CPU file's first chi^2 case through the Python class: the final states of 16384 walkers after 200 sweeps from the all-0
    state against W(n_eq(s)) / sum on open 2 x 3, q = 3 (the twin's number: chi2 = 703.4 on 728 dof, p = 0.737, pooled 0 %)."""
    import tsu
    shape, q, per, wseed, seed = mt.CHI2_CASES[0]
    lnw = mt.chi2_weights(shape, per, wseed)
    m = tsu.PottsMulticanonical(shape[1:], q, mt.CHI2_WALKERS, periodic=False, seed=seed)
    m.weights = lnw
    m.run(mt.CHI2_SWEEPS)
    chi2, dof, p, pooled = mt.weight_chi2(mt.codes(m.spins, q), shape, q, per, lnw)
    assert m.consistent() and int(m.histogram().sum()) == mt.CHI2_WALKERS * mt.CHI2_SWEEPS
    m.close()
    print(f"\nopen 2x3 q=3 on the device: chi2 = {chi2:.1f} on {dof} dof, p = {p:.3f}, pooled {100 * pooled:.2f} %")
    assert p >= 0.01 and pooled <= 0.05


def test_canonical_weights_agree_with_the_heat_bath_of_k10():
    """ln W[n] = n / T makes every walker a canonical Metropolis chain.  Periodic 8 x 8, q = 3, T = 1.2: the mean n_eq of 4096
    independent walkers after 300 sweeps (error sigma / sqrt(4096)) against PottsModel2D under heat bath (200 sweeps discarded,
    4000 measurements 2 sweeps apart, batch means over 20 batches), within 4 combined errors."""
    import tsu
    T, W = 1.2, 4096
    m = tsu.PottsMulticanonical(8, 3, W, periodic=True, seed=21)
    m.weights = np.arange(m.bonds + 1) / T
    m.run(300)
    n = m.energies().astype(np.float64)
    m.close()
    a, ea = n.mean(), n.std(ddof=1) / np.sqrt(W)
    pm = tsu.PottsModel2D(8, 3, temperature=T, seed=22)
    pm.gibbs_update(200)
    rows = pm.run(4000, 2)[:, 0].astype(np.float64)
    pm.close()
    batches = rows.reshape(20, 200).mean(axis=1)
    b, eb = batches.mean(), batches.std(ddof=1) / np.sqrt(20)
    print(f"\n<n_eq>: multicanonical walkers {a:.3f} +- {ea:.3f}, heat bath {b:.3f} +- {eb:.3f}")
    assert abs(a - b) <= 4 * np.hypot(ea, eb)

"""K12 on the GPU (csrc/potts_disorder.hip): heat-bath sweeps and Swendsen-Wang steps on stored couplings bit for bit against the
NumPy twin (tests/helpers/potts_disorder_twin.py) on every route, one layer against the 2-D lattice, constant couplings against K10's
cluster steps, the observables with the energy's bits, split runs, and the enumeration chains of the CPU file on the device.  Every
bit-for-bit case first asserts on the CPU that its inputs hold no fragile decision (the twin's docstring says what that is)."""
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


dt = _load("potts_disorder_twin")
N = dt.N_UPDATES


@pytest.fixture(scope="module")
def hip():
    from tsu import _hip
    return _hip


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in ("TSU_POTTS_SMALL", "TSU_SW3D_TILE", "TSU_SW_TILE"):
        monkeypatch.delenv(name, raising=False)


def _lattice(hip, shape, q, periodic, J, h, spins):
    lat = hip.PottsDisorderLattice(shape, q, periodic)
    lat.set_disorder(J[0], J[1], J[2] if len(J) == 3 else None, h)
    lat.set_spins(spins)
    return lat


def _check_measure(lat, s, q, periodic, J, h):
    """The integers are the twin's (K10's counts); E has the bits of the twin's ordered sum and agrees with the exact sum."""
    n_eq, counts, E = lat.measure()
    w_eq, w_counts = dt.measure(s, q, periodic)
    assert n_eq == w_eq and counts.tolist() == w_counts.tolist()
    want, plain = dt.energy(s, q, periodic, J, h), dt.energy_plain(s, q, periodic, J, h)
    assert np.float64(E).tobytes() == np.float64(want).tobytes(), (E, want)
    assert abs(E - plain) <= 1e-12 * abs(plain)


@pytest.mark.parametrize("case", dt.heat_bath_cases(), ids=dt.case_id)
def test_heat_bath_equals_the_twin_on_both_routes(hip, monkeypatch, case):
    shape, per, q, T = case["shape"], case["periodic"], case["q"], case["T"]
    s, J, h = dt.case_inputs(case)
    want, n_fragile = dt.sweep(s, q, per, J, h, T, N, case["seed"], case["sweep0"], case["replica"], with_fragile=True)
    assert n_fragile == 0 and (want != s).any()
    for route in ("k12_small", "k12_sweep"):
        if route == "k12_sweep":
            monkeypatch.setenv("TSU_POTTS_SMALL", "0")
        lat = _lattice(hip, shape, q, per, J, h, s)
        try:
            assert lat.route() == route
            lat.sweep(T, N, case["seed"], case["sweep0"], case["replica"])
            got = lat.get_spins()
            assert (got == want).all(), (route, int(np.count_nonzero(got != want)))
            assert lat.launch_count() == (1 if route == "k12_small" else 2 * N)
            _check_measure(lat, got, q, per, J, h)
            # a call split in two equals one call, through the counter's wrap where the case starts at 2^32 - 1
            lat.set_spins(s)
            lat.sweep(T, 1, case["seed"], case["sweep0"], case["replica"])
            lat.sweep(T, N - 1, case["seed"], (case["sweep0"] + 1) & 0xFFFFFFFF, case["replica"])
            assert (lat.get_spins() == want).all()
        finally:
            lat.close()


@pytest.mark.parametrize("shape,per", [((5, 19), False), ((6, 32), True)], ids=["5x19-o", "6x32-p"])
@pytest.mark.parametrize("q,field", [(3, True), (8, False)])
def test_one_layer_with_an_open_z_axis_equals_the_2d_lattice(hip, monkeypatch, shape, per, q, field):
    rng = np.random.default_rng(7)
    s = rng.integers(0, q, size=shape).astype(np.int8)
    J, h = dt.random_disorder(shape, per, q, rng, "gaussian", field)
    want, n_fragile = dt.sweep(s, q, per, J, h, 1.1, N, 31, 5, 2, with_fragile=True)
    assert n_fragile == 0
    J3 = (J[0][None], J[1][None], np.zeros((1,) + shape, np.float32))
    h3 = None if h is None else h[:, None]
    for small in (True, False):
        if not small:
            monkeypatch.setenv("TSU_POTTS_SMALL", "0")
        l2 = _lattice(hip, shape, q, per, J, h, s)
        l3 = _lattice(hip, (1,) + shape, q, (False, per, per), J3, h3, s[None])
        try:
            for lat in (l2, l3):
                lat.sweep(1.1, N, 31, 5, 2)
            assert (l2.get_spins() == want).all() and (l3.get_spins()[0] == want).all()
            assert l2.route() == l3.route() == ("k12_small" if small else "k12_sweep")
            assert l2.measure()[2] == l3.measure()[2]
        finally:
            l2.close()
            l3.close()


@pytest.mark.parametrize("case", dt.cluster_cases(), ids=dt.case_id)
def test_cluster_steps_equal_the_twin_on_every_route(hip, monkeypatch, case):
    """Couplings from {0, 1, 2}: one workgroup, then tiles forced to edge 4 (2-D) or to 2 x 3 x 4 (3-D), seams and wraps included."""
    shape, per, q, T = case["shape"], case["periodic"], case["q"], case["T"]
    s, J, _ = dt.case_inputs(case)
    want, n_fragile = dt.cluster_sweep(s, q, per, J, T, N, case["seed"], case["sweep0"], case["replica"], with_fragile=True)
    assert n_fragile == 0 and (want != s).any()
    for route in ("k12_sw_small", "k12_sw_tiles"):
        if route == "k12_sw_tiles":
            monkeypatch.setenv(*(("TSU_SW_TILE", "4") if len(shape) == 2 else ("TSU_SW3D_TILE", "2x3x4")))
        lat = _lattice(hip, shape, q, per, J, None, s)
        try:
            assert lat.route(hip.POTTS_SWENDSEN_WANG) == route
            lat.cluster_sweep(T, N, case["seed"], case["sweep0"], case["replica"])
            got = lat.get_spins()
            assert (got == want).all(), (route, int(np.count_nonzero(got != want)))
            assert lat.launch_count() == (1 if route == "k12_sw_small" else 3 * N)
            _check_measure(lat, got, q, per, J, None)
        finally:
            lat.close()


@pytest.mark.parametrize("case", dt.cluster_cases()[1::3], ids=dt.case_id)
def test_constant_couplings_take_k10s_cluster_steps(hip, monkeypatch, case):
    """J_b = 1 on every bond: the same threshold formula as K10's, so the same colours from the same colours, seed and step."""
    shape, per, q, T = case["shape"], case["periodic"], case["q"], case["T"]
    s, _, _ = dt.case_inputs(case)
    J = dt.constant_couplings(shape, per, 1.0)
    assert dt.cluster_sweep(s, q, per, J, T, N, case["seed"], case["sweep0"], case["replica"], with_fragile=True)[1] == 0
    for tiles in (False, True):
        if tiles:
            monkeypatch.setenv(*(("TSU_SW_TILE", "4") if len(shape) == 2 else ("TSU_SW3D_TILE", "2x3x4")))
        lat = _lattice(hip, shape, q, per, J, None, s)
        k10 = hip.PottsLattice(shape[0], shape[1], q, per) if len(shape) == 2 else hip.PottsLattice3D(*shape, q, per)
        try:
            k10.set_model(1.0)
            k10.set_spins(s)
            k10.cluster_sweep(T, N, case["seed"], case["sweep0"], case["replica"])
            lat.cluster_sweep(T, N, case["seed"], case["sweep0"], case["replica"])
            assert (lat.get_spins() == k10.get_spins()).all() and (lat.get_spins() != s).any()
            n_eq, counts, E = lat.measure()
            k_eq, k_counts = k10.measure()
            assert n_eq == k_eq and counts.tolist() == k_counts.tolist() and E == -float(n_eq)
        finally:
            lat.close()
            k10.close()


def test_cluster_steps_refuse_a_negative_bond_and_a_field(hip):
    rng = np.random.default_rng(9)
    s = rng.integers(0, 3, size=(8, 12)).astype(np.int8)
    J, _ = dt.random_disorder((8, 12), True, 3, rng, "012", False)
    neg = (J[0].copy(), J[1])
    neg[0][3, 4] = -0.5
    h = np.zeros((3, 8, 12), np.float32)
    h[1, 2, 2] = 0.25
    for Jx, hx in ((neg, None), (J, h)):
        lat = _lattice(hip, (8, 12), 3, True, Jx, hx, s)
        try:
            with pytest.raises(hip.UnsupportedError):
                lat.cluster_sweep(1.5, 2, 1)
            with pytest.raises(hip.UnsupportedError):
                lat.run(1.5, 2, 1, hip.POTTS_SWENDSEN_WANG, 1)
            assert (lat.get_spins() == s).all() and lat.launch_count() == 0
            lat.sweep(1.5, 1, 1)  # heat-bath sweeps take either
            assert (lat.get_spins() == dt.sweep(s, 3, True, Jx, hx, 1.5, 1, 1)).all()
        finally:
            lat.close()
    lat = _lattice(hip, (8, 12), 3, True, J, 0 * h, s)  # a field that is given and all zero allows the steps
    try:
        lat.cluster_sweep(1.5, 2, 1)
        assert (lat.get_spins() == dt.cluster_sweep(s, 3, True, J, 1.5, 2, 1)).all()
        with pytest.raises(ValueError):
            lat.sweep(0.0, 1, 1)
        with pytest.raises(ValueError):
            lat.sweep(float("nan"), 1, 1)
    finally:
        lat.close()
    lat = hip.PottsDisorderLattice((8, 12), 3, True)
    try:
        with pytest.raises(ValueError):  # no disorder yet
            lat.sweep(1.0, 1, 1)
        with pytest.raises(ValueError):  # an open axis's last column must be 0
            hip.PottsDisorderLattice((3, 5), 3, False).set_disorder(np.ones((3, 5)), np.zeros((3, 5)))
        with pytest.raises(ValueError):  # a 2-D lattice takes no J_layer
            lat.set_disorder(J[0], J[1], J[0])
    finally:
        lat.close()


@pytest.mark.parametrize("shape,per,q", [((130, 130), False, 3), ((18, 32, 32), True, 8), ((1040, 260), True, 2)],
                         ids=["130x130-o", "18x32x32-p", "1040x260-p"])
def test_measure_beyond_one_workgroup_equals_k10_and_the_twin(hip, shape, per, q):
    """More than 16384 sites: k12_sweep and a grid of many partials; 1040 x 260 fills all 1024 partials and strides the sites.  The
    integers equal K10's measure on the same colours."""
    rng = np.random.default_rng(11)
    s = rng.integers(0, q, size=shape).astype(np.int8)
    J, h = dt.random_disorder(shape, per, q, rng, "gaussian", True)
    want, n_fragile = dt.sweep(s, q, per, J, h, 1.2, 1, 77, 0, 0, with_fragile=True)
    assert n_fragile == 0
    lat = _lattice(hip, shape, q, per, J, h, s)
    k10 = hip.PottsLattice(shape[0], shape[1], q, per) if len(shape) == 2 else hip.PottsLattice3D(*shape, q, per)
    try:
        assert lat.route() == "k12_sweep"
        lat.sweep(1.2, 1, 77)
        got = lat.get_spins()
        assert (got == want).all()
        _check_measure(lat, got, q, per, J, h)
        k10.set_spins(got)
        n_eq, counts, E = lat.measure()
        k_eq, k_counts = k10.measure()
        assert n_eq == k_eq and counts.tolist() == k_counts.tolist()
        assert lat.measure()[2] == E  # the same bits on every call
    finally:
        lat.close()
        k10.close()


@pytest.mark.parametrize("algorithm", ["heat_bath", "swendsen_wang"])
@pytest.mark.parametrize("shape,per", [((6, 32), True), ((3, 5, 7), False)], ids=["6x32-p", "3x5x7-o"])
def test_a_run_split_in_two_equals_one_run(hip, shape, per, algorithm):
    q, T, seed = 3, 1.4, 2 ** 64 - 59
    hb = algorithm == "heat_bath"
    alg = hip.POTTS_HEAT_BATH if hb else hip.POTTS_SWENDSEN_WANG
    rng = np.random.default_rng(13)
    s = rng.integers(0, q, size=shape).astype(np.int8)
    J, h = dt.random_disorder(shape, per, q, rng, "gaussian" if hb else "012", hb)
    c0 = 2 ** 32 - 3 if hb else 40
    one = _lattice(hip, shape, q, per, J, h, s)
    two = _lattice(hip, shape, q, per, J, h, s)
    try:
        one.run(T, 4, 2, alg, seed, c0, 1)
        rows, E = one.record()
        two.run(T, 1, 2, alg, seed, c0, 1)
        r1, e1 = two.record()
        two.run(T, 3, 2, alg, seed, (c0 + 2) & 0xFFFFFFFF, 1)
        r2, e2 = two.record()
        assert rows.shape == (4, 9) and E.shape == (4,)
        assert (np.concatenate([r1, r2]) == rows).all() and np.concatenate([e1, e2]).tobytes() == E.tobytes()
        assert (one.get_spins() == two.get_spins()).all()
        # the rows are the twin's, measurement by measurement
        t = s
        for k in range(4):
            if hb:
                t, f = dt.sweep(t, q, per, J, h, T, 2, seed, (c0 + 2 * k) & 0xFFFFFFFF, 1, with_fragile=True)
            else:
                t, f = dt.cluster_sweep(t, q, per, J, T, 2, seed, c0 + 2 * k, 1, with_fragile=True)
            assert f == 0
            n_eq, counts = dt.measure(t, q, per)
            assert rows[k, 0] == n_eq and rows[k, 1:1 + q].tolist() == counts.tolist() and (rows[k, 1 + q:] == 0).all()
            assert np.float64(E[k]).tobytes() == np.float64(dt.energy(t, q, per, J, h)).tobytes()
        assert (one.get_spins() == t).all()
    finally:
        one.close()
        two.close()


def _device_codes(lat, q, update, n_discard, n_states, every):
    update(n_discard, 0)
    codes = []
    for k in range(n_states):
        update(every, n_discard + k * every)
        codes.append(dt.state_code(lat.get_spins(), q))
    return codes


# chi^2 of the twin's chains (tests/test_potts_disorder_cpu.py records them with dof, p and the pooled share, and asserts that no
# decision of the chains is fragile); the device repeats them
HEAT_BATH_CHI2 = {"2x3-q3": "493.6", "2x2x2-q2": "284.5"}
CLUSTER_CHI2 = {"2x3-q3": "543.7"}


def _enum_id(case):
    return "x".join(map(str, case[0])) + f"-q{case[1]}"


@pytest.mark.parametrize("case", dt.ENUMERATION_HEAT_BATH, ids=_enum_id)
def test_heat_bath_enumeration_on_the_device(hip, case):
    """The CPU test's chains on the device: the first 50 recorded states equal the twin's, and the 20 000 states give the twin's
    chi^2 to the digit and pass the same check."""
    shape, q, per, kind, field, T, dseed, seed = case
    J, h = dt.enumeration_disorder(case)
    lat = _lattice(hip, shape, q, per, J, h, np.zeros(shape, np.int8))
    try:
        codes = _device_codes(lat, q, lambda n, c0: lat.sweep(T, n, seed, c0), dt.N_DISCARD, dt.N_STATES, dt.EVERY)
    finally:
        lat.close()
    s, _, _ = dt.chain(np.zeros(shape, np.int8), q, per, J, h, T, dt.N_DISCARD, seed)
    _, want, _ = dt.chain(s, q, per, J, h, T, 50 * dt.EVERY, seed, sweep0=dt.N_DISCARD, record_every=dt.EVERY)
    assert codes[:50] == want
    chi2, dof, p, pooled = dt.boltzmann_chi2(codes, shape, q, per, J, h, T)
    print(f"\n{_enum_id(case)}: chi2 = {chi2:.1f} on {dof} dof, p = {p:.3f}, pooled {100 * pooled:.2f} %")
    assert f"{chi2:.1f}" == HEAT_BATH_CHI2[_enum_id(case)] and p >= 0.01 and pooled <= 0.05


@pytest.mark.parametrize("case", dt.ENUMERATION_CLUSTER, ids=_enum_id)
def test_cluster_enumeration_on_the_device(hip, case):
    shape, q, per, kind, field, T, dseed, seed = case
    J, _ = dt.enumeration_disorder(case)
    lat = _lattice(hip, shape, q, per, J, None, np.zeros(shape, np.int8))
    try:
        codes = _device_codes(lat, q, lambda n, c0: lat.cluster_sweep(T, n, seed, c0), dt.N_DISCARD, dt.N_STATES, dt.EVERY)
    finally:
        lat.close()
    s, _, _ = dt.cluster_chain(np.zeros(shape, np.int8), q, per, J, T, dt.N_DISCARD, seed)
    _, want, _ = dt.cluster_chain(s, q, per, J, T, 50 * dt.EVERY, seed, step0=dt.N_DISCARD, record_every=dt.EVERY)
    assert codes[:50] == want
    chi2, dof, p, pooled = dt.boltzmann_chi2(codes, shape, q, per, J, None, T)
    print(f"\n{_enum_id(case)}: chi2 = {chi2:.1f} on {dof} dof, p = {p:.3f}, pooled {100 * pooled:.2f} %")
    assert f"{chi2:.1f}" == CLUSTER_CHI2[_enum_id(case)] and p >= 0.01 and pooled <= 0.05


def test_model_facade_and_scan(hip):
    import tsu
    from tsu.models import potts
    rng = np.random.default_rng(17)
    shape, q = (6, 32), 3
    J, h = dt.random_disorder(shape, True, q, rng, "gaussian", True)
    m = tsu.PottsModel2D(shape, q, temperature=1.3, seed=21, couplings=J, site_field=np.moveaxis(h, 0, -1))
    try:
        s = m.spins
        assert (s == np.random.default_rng(21).integers(0, q, size=shape)).all() and m.route() == "k12_small"
        m.gibbs_update(2)
        want, f = dt.sweep(s, q, True, J, h, 1.3, 2, 21, with_fragile=True)
        assert f == 0 and (m.spins == want).all() and m.sweep_count == 2
        assert m.energy() == dt.energy(want, q, True, J, h) and m.equal_bonds() == dt.measure(want, q, True)[0]
        assert m.colour_counts().tolist() == dt.measure(want, q, True)[1].tolist() and 0.0 <= m.order_parameter() <= 1.0
        rows, E = m.run(3, 2)
        assert rows.shape == (3, 1 + q) and E.shape == (3,) and m.sweep_count == 8 and E[-1] == m.energy()
        with pytest.raises(hip.UnsupportedError):
            m.cluster_update(1)
        pos = dt.random_disorder(shape, True, q, rng, "012", False)[0]
        m.set_disorder(couplings=pos, site_field=np.zeros(shape + (q,)))
        before = m.spins
        m.cluster_update(2)
        assert (m.spins == dt.cluster_sweep(before, q, True, pos, 1.3, 2, 21)).all() and m.cluster_count == 2
        m.equilibrate(0.8, 2)
        assert m.temperature == 0.8 and m.launch_count() > 0
    finally:
        m.close()
    m3 = tsu.PottsModel3D((2, 4, 16), 2, temperature=2.0, seed=5, initial=1, site_field=np.zeros((2, 4, 16, 2)), coupling=0.5)
    try:
        assert m3.energy() == -0.5 * 3 * 128 and m3.route() == "k12_small"  # every bond of the periodic lattice, once per stored value
    finally:
        m3.close()
    bim = tuple(np.where(rng.random(size=(8, 8)) < 0.5, 1.0, 2.0) for _ in range(2))
    res = potts.potts_temperature_scan(8, 3, [0.5, 5.0], n_equilibrate=20, n_measure=10, algorithm="swendsen_wang", seed=3, couplings=bim)
    assert set(res) == {"energy", "order_parameter", "specific_heat", "susceptibility", "binder", "temperatures"}
    assert res["energy"][0] < res["energy"][1] < 0 and res["order_parameter"][0] > 0.9 > res["order_parameter"][1]

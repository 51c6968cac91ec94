"""K7 disordered lattice on the host: the NumPy twin (tests/helpers/disorder_twin.py) against the pinned oracle with constant
dyadic disorder, its site uniforms against the oracle's, the near-tie construction, and the Python layer's validation, which
must refuse bad disorder before the device is touched (no GPU needed)."""
import importlib.util
import math
import os

import numpy as np
import pytest

from oracle import oracle as ora

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("disorder_twin", os.path.join(HERE, "helpers", "disorder_twin.py"))
twin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(twin)

TC = 2.0 / math.log(1.0 + math.sqrt(2.0))
SHAPES = [(8, 8, True), (6, 10, True), (5, 7, False), (1, 9, False)]
DYADIC = [(1.0, 0.0), (0.5, 0.25), (-0.75, 0.5)]


@pytest.mark.parametrize("rows,cols", [(8, 8), (6, 10), (5, 7), (1, 9), (9, 1), (3, 40)])
def test_twin_site_uniforms_match_oracle(rows, cols):
    for hs, seed, replica in ((0, 1, 0), (7, 0xDEADBEEF12345, 3), (2 ** 31, 5, 255)):
        assert (twin.site_uniforms(rows, cols, hs, seed, replica) == ora.ising2d_site_uniforms(rows, cols, hs, seed, replica)).all()


@pytest.mark.parametrize("rows,cols,periodic", SHAPES)
@pytest.mark.parametrize("J,h", DYADIC)
@pytest.mark.parametrize("T", [TC, 1.5, 0.4])
def test_twin_equals_k1_oracle_on_constant_dyadic_disorder(rows, cols, periodic, J, h, T):
    """2 (J sum s + h) is exact for dyadic (J, h): x, thr and the spins equal K1's table route bit for bit."""
    s0 = ora.ising2d_randomize(rows, cols, 17)
    jr, jd, hh = twin.uniform_disorder(rows, cols, periodic, J, h)
    table = ora.ising2d_thresholds(J, h, T, ora.MODE_PHYSICAL)
    want, got = s0, s0
    for sweep0, n in ((0, 3), (3, 5)):
        want = ora.ising2d_sweep(want, periodic, table, n, 41, sweep0, 2)
        got = twin.sweep(got, periodic, jr, jd, hh, T, n, 41, sweep0, 2)
        assert (got == want).all(), (rows, cols, periodic, J, h, T, sweep0)


def test_twin_local_field_order_and_skipped_terms():
    # open 3 x 3: the corner has two neighbours, the centre four; values chosen so the order is visible in float64
    s = np.array([[1, -1, 1], [-1, 1, 1], [1, 1, -1]], np.int8)
    jr = np.zeros((3, 3), np.float32)
    jd = np.zeros((3, 3), np.float32)
    jr[:, :2] = np.float32(1e8)
    jd[:2, :] = np.float32(1.0)
    h = np.full((3, 3), np.float32(0.25))
    f = twin.local_field(s, False, jr, jd, h)
    up, dn, lf, rt = 1.0 * s[0, 1], 1.0 * s[2, 1], 1e8 * s[1, 0], 1e8 * s[1, 2]
    assert f[1, 1] == (((up + dn) + lf) + rt) + 0.25
    assert f[0, 0] == (1.0 * s[1, 0] + 1e8 * s[0, 1]) + 0.25


def test_near_tie_field_puts_decisions_on_their_thresholds():
    rows, cols, T = 64, 48, 1.0
    h = twin.tie_field(rows, cols, T, seed=9)
    z = np.zeros((rows, cols), np.float32)
    stats = {}
    twin.sweep(np.ones((rows, cols), np.int8), True, z, z, h, T, 1, 9, 0, 0, stats=stats)
    assert stats["sites"] == rows * cols
    assert stats["near"] > 0.9 * stats["sites"], stats


def test_energy_and_overlap_twins():
    rng = np.random.default_rng(1)
    s = np.where(rng.random((6, 10)) < 0.5, 1, -1).astype(np.int8)
    jr, jd, h = (rng.normal(size=(6, 10)).astype(np.float32) for _ in range(3))
    e = 0.0
    for r in range(6):
        for c in range(10):
            e -= float(jr[r, c]) * s[r, c] * s[r, (c + 1) % 10] + float(jd[r, c]) * s[r, c] * s[(r + 1) % 6, c] + float(h[r, c]) * s[r, c]
    assert twin.energy(s, True, jr, jd, h) == pytest.approx(e, rel=1e-12)
    assert twin.overlap(s, -s) == -60


# ---------------------------------------------------------------- validation before the device is touched
@pytest.fixture
def no_device(monkeypatch):
    from tsu import _hip

    def boom(*a, **k):
        raise AssertionError("the device was touched before validation")
    monkeypatch.setattr(_hip, "Lattice", boom)
    return _hip


def _arrays(rows, cols, periodic=True, J=1.0):
    return twin.uniform_disorder(rows, cols, periodic, J, 0.0)


@pytest.mark.parametrize("kw", [
    dict(couplings=_arrays(8, 8)[:2], bias_mode="compat"),
    dict(field=np.zeros((8, 8)), bias_mode="compat"),
    dict(couplings=_arrays(8, 8)[:2], coupling=2.0),
    dict(field=np.zeros((8, 8)), external_field=0.5),
    dict(couplings=_arrays(8, 6)[:2]),
    dict(field=np.zeros((6, 8))),
    dict(couplings=(np.full((8, 8), np.nan), np.ones((8, 8)))),
    dict(field=np.full((8, 8), np.inf)),
    dict(field=np.full((8, 8), 1e300)),
    dict(couplings=(np.ones((8, 8)),)),
    dict(couplings=(np.ones((8, 8)), np.ones((8, 8))), periodic=False),
])
def test_model_validation_precedes_device(no_device, kw):
    from tsu.models.ising import IsingModel2D
    with pytest.raises(ValueError):
        IsingModel2D(8, temperature=2.0, seed=1, **kw)


def test_open_lattice_boundary_rule(no_device):
    from tsu.models.ising import _disorder_arrays
    jr, jd, _ = _arrays(5, 7, periodic=False)
    out = _disorder_arrays(5, 7, False, 1.0, 0.0, "physical", (jr, jd), None)
    assert out[2] is None and out[0].dtype == np.float32
    bad = jr.copy()
    bad[2, -1] = 0.5
    with pytest.raises(ValueError, match="last column"):
        _disorder_arrays(5, 7, False, 1.0, 0.0, "physical", (bad, jd), None)
    bad = jd.copy()
    bad[-1, 3] = -1.0
    with pytest.raises(ValueError, match="last row"):
        _disorder_arrays(5, 7, False, 1.0, 0.0, "physical", (jr, bad), None)
    # couplings=None on an open lattice: the scalar coupling with the boundary zeros filled in
    jr2, jd2, h2 = _disorder_arrays(5, 7, False, 0.5, 0.25, "physical", None, None)
    assert (jr2[:, -1] == 0).all() and (jd2[-1] == 0).all() and (jr2[:, :-1] == 0.5).all() and (h2 == 0.25).all()


def test_scan_validation_precedes_device(no_device):
    from tsu.models.ising import temperature_scan
    jr, jd, _ = _arrays(8, 8)
    with pytest.raises(no_device.UnsupportedError):
        temperature_scan(8, [1.0, 2.0], couplings=(jr, jd), algorithm="swendsen_wang")
    with pytest.raises(ValueError):
        temperature_scan(8, [1.0, 2.0], replicas=3)
    with pytest.raises(ValueError):
        temperature_scan(8, [1.0, 2.0], couplings=(jr, jd), coupling=2.0)
    with pytest.raises(ValueError):
        temperature_scan(8, [1.0, 2.0], field=np.zeros((8, 8)), bias_mode="compat")
    with pytest.raises(ValueError):
        temperature_scan(8, [1.0, 2.0], field=np.zeros((4, 8)))

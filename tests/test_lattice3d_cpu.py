"""K8 3-D disordered lattice on the host: the NumPy twin (tests/helpers/lattice3d_twin.py) against K7's twin at D = 1, its field
order and skipped terms, the near-tie constructions, the energy and overlap twins, a prefix of the exact-enumeration run, the
Python layer's validation (which must refuse bad input before the device is touched), and the C ABI's symbols (no GPU needed)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


twin = _load("lattice3d_twin")
twin2 = _load("disorder_twin")


def _disorder2d(kind, rows, cols, periodic, seed):
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        jr, jd, h = (rng.normal(size=(rows, cols)) for _ in range(3))
    elif kind == "pmJ":
        jr, jd = (np.where(rng.random((rows, cols)) < 0.5, 1.0, -1.0) for _ in range(2))
        h = np.zeros((rows, cols))
    else:  # uniform J, Gaussian h (random-field)
        jr, jd = np.ones((rows, cols)), np.ones((rows, cols))
        h = rng.normal(scale=0.7, size=(rows, cols))
    jr, jd, h = jr.astype(np.float32), jd.astype(np.float32), h.astype(np.float32)
    if not periodic:
        jr[:, -1] = 0.0
        jd[-1, :] = 0.0
    return jr, jd, h


@pytest.mark.parametrize("rows,cols,periodic", [(5, 37, False), (6, 40, True)])
@pytest.mark.parametrize("kind", ["gauss", "pmJ", "rfim"])
def test_twin_with_one_layer_is_k7s_twin(rows, cols, periodic, kind):
    """D = 1, p_z = False: the z terms vanish, rho = r, and the rule is K7's."""
    jr, jd, h = _disorder2d(kind, rows, cols, periodic, 3 + rows)
    s0 = np.where(np.random.default_rng(1).random((rows, cols)) < 0.5, 1, -1).astype(np.int8)
    shape = (1, rows, cols)
    jl = np.zeros(shape, np.float32)
    for replica, T in ((0, 1.3), (2, 0.4)):
        want = twin2.sweep(s0, periodic, jr, jd, h, T, 4, 41, 2, replica)
        got = twin.sweep(s0.reshape(shape), (False, periodic, periodic), jr.reshape(shape), jd.reshape(shape), jl, h.reshape(shape),
                         T, 4, 41, 2, replica)
        assert (got.reshape(rows, cols) == want).all(), (rows, cols, periodic, kind, T)


def test_twin_site_uniforms_use_the_global_row():
    u = twin.site_uniforms((3, 5, 37), 7, 0xDEADBEEF12345, 3)
    assert (u == twin2.site_uniforms(15, 37, 7, 0xDEADBEEF12345, 3).reshape(3, 5, 37)).all()
    assert (twin.colours((2, 2, 2))[1] == [[1, 0], [0, 1]]).all()


def test_twin_local_field_order_and_skipped_terms():
    # open 3 x 3 x 3: the centre has six neighbours, the corner three; magnitudes chosen so the order is visible in float64
    rng = np.random.default_rng(4)
    shape = (3, 3, 3)
    s = np.where(rng.random(shape) < 0.5, 1, -1).astype(np.int8)
    jr, jd, jl, h = twin.uniform_disorder(shape, False, 1.0, 0.25)
    jr[jr != 0] = np.float32(1e8)
    jd[jd != 0] = np.float32(3.0)
    jl[jl != 0] = np.float32(1e-3)
    f = twin.local_field(s, False, jr, jd, jl, h)
    a, b = float(np.float32(1e-3)) * s[0, 1, 1], float(np.float32(1e-3)) * s[2, 1, 1]
    c, d = 3.0 * s[1, 0, 1], 3.0 * s[1, 2, 1]
    e, g = 1e8 * s[1, 1, 0], 1e8 * s[1, 1, 2]
    assert f[1, 1, 1] == (((((a + b) + c) + d) + e) + g) + 0.25
    assert f[0, 0, 0] == ((float(np.float32(1e-3)) * s[1, 0, 0] + 3.0 * s[0, 1, 0]) + 1e8 * s[0, 0, 1]) + 0.25
    # mixed boundaries: z periodic wraps, r open skips
    jr, jd, jl, h = twin.uniform_disorder((4, 3, 4), (True, False, True), 1.0, 0.0)
    s = np.where(rng.random((4, 3, 4)) < 0.5, 1, -1).astype(np.int8)
    f = twin.local_field(s, (True, False, True), jr, jd, jl, h)
    assert f[0, 0, 0] == float(s[3, 0, 0]) + s[1, 0, 0] + s[0, 1, 0] + s[0, 0, 3] + s[0, 0, 1]
    # a site without any neighbour: f = h exactly
    one = np.ones((1, 1, 1), np.int8)
    z = np.zeros((1, 1, 1), np.float32)
    assert twin.local_field(one, False, z, z, z, np.full((1, 1, 1), np.float32(-0.5)))[0, 0, 0] == -0.5


@pytest.mark.parametrize("T", [0.4, 2.27])
def test_near_tie_field_puts_decisions_on_their_thresholds(T):
    shape = (3, 5, 37)
    h = twin.tie_field(shape, T, seed=9)
    z = np.zeros(shape, np.float32)
    stats = {}
    twin.sweep(np.ones(shape, np.int8), False, z, z, z, h, T, 1, 9, 0, 0, stats=stats)
    assert stats["sites"] == 3 * 5 * 37
    assert stats["near"] > 0.9 * stats["sites"], stats


def test_near_tie_field_with_couplings_puts_seven_term_sums_on_their_thresholds():
    shape, per, T = (4, 6, 40), True, 1.1
    rng = np.random.default_rng(8)
    jr, jd, jl = (rng.normal(size=shape).astype(np.float32) for _ in range(3))
    s0 = np.where(rng.random(shape) < 0.5, 1, -1).astype(np.int8)
    h = twin.tie_field(shape, T, 9, 0, spins=s0, periodic=per, couplings=(jr, jd, jl))
    stats = {}
    twin.sweep(s0, per, jr, jd, jl, h, T, 1, 9, 0, 0, stats=stats)
    assert stats["near"] > 0.9 * stats["sites"], stats


def test_energy_and_overlap_twins():
    rng = np.random.default_rng(1)
    shape = (4, 6, 10)
    s = np.where(rng.random(shape) < 0.5, 1, -1).astype(np.int8)
    jr, jd, jl, h = (rng.normal(size=shape).astype(np.float32) for _ in range(4))
    e = 0.0
    for z in range(4):
        for r in range(6):
            for c in range(10):
                e -= s[z, r, c] * (float(jr[z, r, c]) * s[z, r, (c + 1) % 10] + float(jd[z, r, c]) * s[z, (r + 1) % 6, c]
                                   + float(jl[z, r, c]) * s[(z + 1) % 4, r, c] + float(h[z, r, c]))
    got, total = twin.energy_terms(s, True, jr, jd, jl, h)
    assert abs(got - e) <= 1e-12 * total
    # open r axis: the wrap bonds of that axis are dropped whatever J says
    e_open = e + sum(float(jd[z, 5, c]) * s[z, 5, c] * s[z, 0, c] for z in range(4) for c in range(10))
    assert abs(twin.energy(s, (True, False, True), jr, jd, jl, h) - e_open) <= 1e-12 * total
    assert twin.overlap(s, -s) == -240


def test_enumeration_prefix_samples_the_boltzmann_distribution():
    """The first 2 000 recorded states of the exact-enumeration case (2, 2, 2), T = 2.0, seed 11, dseed 3 (the GPU test runs all
    20 000 on the device): same criterion, p >= 0.01 and a pooled share <= 5 % -- at n = 2 000 fewer states reach an expected count
    of 5, so the share is asserted only where the issue states it, for the full run."""
    shape, T, seed = (2, 2, 2), 2.0, 11
    d = twin.enumeration_disorder(shape, 3)
    assert all((a[sl] == 0).all() for a, sl in zip(d[:3], ((slice(None), slice(None), -1), (slice(None), -1), (-1,))))
    s = twin.sweep(np.ones(shape, np.int8), False, *d, T, 100, seed, 0)
    codes, sweeps = [], 100
    for _ in range(2000):
        s = twin.sweep(s, False, *d, T, 4, seed, sweeps)
        sweeps += 4
        codes.append(twin.state_code(s))
    chi2, dof, p, pooled = twin.boltzmann_chi2(codes, shape, d, T)
    print(f"chi2 = {chi2:.1f} on {dof} d.o.f., p = {p:.3f}, pooled share {pooled:.3%}")
    assert p >= 0.01, (chi2, dof, p)


# ---------------------------------------------------------------- validation before the device is touched
@pytest.fixture
def no_device(monkeypatch):
    from tsu import _hip

    def boom(*a, **k):
        raise AssertionError("the device was touched before validation")
    monkeypatch.setattr(_hip, "Lattice3D", boom)
    return _hip


def _arrays(shape, periodic=True, J=1.0):
    return twin.uniform_disorder(shape, periodic, J, 0.0)[:3]


S = (4, 6, 8)
BAD = [
    dict(couplings=_arrays((4, 6, 6))),                                         # wrong shape
    dict(couplings=_arrays(S)[:2]),                                             # a pair, not a triple
    dict(field=np.zeros((6, 4, 8))),
    dict(couplings=(np.full(S, np.nan),) + _arrays(S)[1:]),                     # non-finite
    dict(couplings=_arrays(S)[:2] + (np.full(S, np.inf),)),
    dict(field=np.full(S, -np.inf)),
    dict(field=np.full(S, 1e300)),                                              # fp32 overflow
    dict(couplings=(np.full(S, 1e39),) + _arrays(S)[1:]),
    dict(couplings=_arrays(S), periodic=(True, True, False)),                   # non-zero last slice on an open axis
    dict(couplings=_arrays(S), periodic=(True, False, True)),
    dict(couplings=_arrays(S), periodic=(False, True, True)),
    dict(couplings=_arrays(S), periodic=False),
    dict(couplings=_arrays(S), coupling=2.0),                                   # arrays and a scalar
    dict(field=np.zeros(S), external_field=0.5),
    dict(temperature=0.0),
    dict(temperature=-1.0),
    dict(initial="sideways"),
    dict(periodic=(True, True)),
]


@pytest.mark.parametrize("kw", BAD)
def test_model_validation_precedes_device(no_device, kw):
    from tsu.models.ising import IsingModel3D
    kw = dict(kw)
    kw.setdefault("temperature", 2.0)
    with pytest.raises(ValueError):
        IsingModel3D(S, seed=1, **kw)


@pytest.mark.parametrize("size,periodic", [((5, 6, 8), True), ((4, 6, 7), True), ((4, 2, 8), True), ((2, 2, 2), True),
                                           ((4, 6, 2), (False, False, True)), ((4, 3, 8), (False, True, False))])
def test_periodic_axis_rule_precedes_device(no_device, size, periodic):
    """A periodic axis needs an even length >= 4 (length 2 would be a double bond): refused, not approximated."""
    from tsu.models.ising import IsingModel3D, temperature_scan_3d
    with pytest.raises(no_device.UnsupportedError):
        IsingModel3D(size, temperature=2.0, periodic=periodic, seed=1)
    with pytest.raises(no_device.UnsupportedError):
        temperature_scan_3d(size, [1.0, 2.0], periodic=periodic)


def test_open_axis_rule_and_uniform_arrays(no_device):
    from tsu.models.ising import _disorder_arrays_3d
    shape, per = (3, 5, 7), (False, False, False)
    jr, jd, jl = _arrays(shape, periodic=False)
    out = _disorder_arrays_3d(shape, per, 1.0, 0.0, (jr, jd, jl), None)
    assert out[3] is None and all(a.dtype == np.float32 for a in out[:3])
    for k, (name, index) in enumerate((("last column", (1, 2, -1)), ("last row", (1, -1, 3)), ("last layer", (-1, 2, 3)))):
        bad = [jr.copy(), jd.copy(), jl.copy()]
        bad[k][index] = 0.5
        with pytest.raises(ValueError, match=name):
            _disorder_arrays_3d(shape, per, 1.0, 0.0, tuple(bad), None)
    # couplings=None: the scalar coupling with the boundary zeros filled in, per axis
    jr2, jd2, jl2, h2 = _disorder_arrays_3d((4, 5, 7), (True, False, False), 0.5, 0.25, None, None)
    assert (jr2[:, :, -1] == 0).all() and (jd2[:, -1] == 0).all() and (jl2 == 0.5).all() and (jr2[:, :, :-1] == 0.5).all()
    assert (h2 == 0.25).all() and h2.dtype == np.float32


def test_scan_validation_precedes_device(no_device):
    from tsu.models.ising import temperature_scan_3d
    jr, jd, jl = _arrays(S)
    with pytest.raises(ValueError):
        temperature_scan_3d(S, [1.0, 2.0], replicas=3)
    with pytest.raises(ValueError):
        temperature_scan_3d(S, [1.0, 2.0], couplings=(jr, jd, jl), coupling=2.0)
    with pytest.raises(ValueError):
        temperature_scan_3d(S, [1.0, 2.0], field=np.zeros((4, 8, 6)))
    with pytest.raises(ValueError):
        temperature_scan_3d(S, [1.0, 0.0])
    with pytest.raises(ValueError):
        temperature_scan_3d(S, [1.0, 2.0], couplings=(jr, jd, jl), periodic=(True, False, True))


def test_disorder_is_rounded_once_to_float32(monkeypatch):
    """`disorder` returns the rounded copies the device got (a stand-in handle records what it is given)."""
    from tsu import _hip
    from tsu.models.ising import IsingModel3D
    seen = {}

    class Fake:
        def __init__(self, *a):
            seen["create"] = a

        def randomize(self, seed, replica=0):
            seen["seed"] = seed

        def set_disorder(self, *d):
            seen["disorder"] = d

    monkeypatch.setattr(_hip, "Lattice3D", Fake)
    rng = np.random.default_rng(0)
    arrays = [rng.normal(size=S) for _ in range(4)]
    np.random.seed(5)
    m = IsingModel3D(S, temperature=1.5, couplings=arrays[:3], field=arrays[3])
    assert seen["create"] == (4, 6, 8, (True, True, True)) and seen["seed"] == m.seed and m.sweep_count == 0
    np.random.seed(5)
    assert m.seed == int(np.random.randint(0, 2 ** 31 - 1)) | (int(np.random.randint(0, 2 ** 31 - 1)) << 31)
    for got, sent, a in zip(m.disorder, seen["disorder"], arrays):
        assert got.dtype == np.float32 and (got == a.astype(np.float32)).all() and (sent == got).all()
    m.disorder[0][:] = 0  # a copy: the model's own arrays are untouched
    assert (m.disorder[0] == arrays[0].astype(np.float32)).all()


# ---------------------------------------------------------------- the C ABI
NAMES = ["tsu_ising3d_create", "tsu_ising3d_destroy", "tsu_ising3d_set_spins", "tsu_ising3d_get_spins", "tsu_ising3d_randomize",
         "tsu_ising3d_fill", "tsu_ising3d_set_disorder", "tsu_ising3d_sweep", "tsu_ising3d_energy", "tsu_ising3d_sum_spins",
         "tsu_ising3d_overlap", "tsu_ising3d_launch_count"]


def test_symbols_in_header_library_and_signatures():
    from tsu import _hip
    header = open(os.path.join(ROOT, "include", "tsu_hip.h")).read()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for n in NAMES:
        assert n + "(" in header, n
        assert hasattr(lib, n), n
        assert n in _hip.SIGNATURES, n
    assert sorted(n for n in _hip.SIGNATURES if n.startswith("tsu_ising3d_")) == sorted(NAMES)
    import tsu
    import tsu.models
    for mod in (tsu, tsu.models):
        assert hasattr(mod, "IsingModel3D") and hasattr(mod, "temperature_scan_3d")
        assert "IsingModel3D" in mod.__all__ and "temperature_scan_3d" in mod.__all__



def test_decision_rule_is_written_once():
    """K7 and K8, single lattices and walker groups, run one octet body (disorder_dev.h): over all of csrc the exact threshold and
    the screen are each called once, the lo16 draw does not appear in either dimension's file, and there is one energy lane and one
    ensemble struct.  Comments are not code: they are dropped before counting."""
    import re
    csrc = os.path.join(ROOT, "tsu-emulator_amd", "csrc")
    raw = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))}
    code = "\n".join(re.sub(r"//[^\n]*", "", s) for s in raw.values())
    for fn, ret in (("exact_thr", "uint64_t"), ("screen", "int")):
        defs = len(re.findall(rf"\b{ret}\s+{fn}\s*\(", code))
        uses = len(re.findall(rf"\b{fn}\s*\(", code)) - defs
        assert (defs, uses) == (1, 1), (fn, defs, uses)
    for name in ("ising2d_disorder.hip", "ising3d.hip"):
        assert "TSU_TAG_ISING_LO" not in raw[name], name
    assert set(re.findall(r"\b\w*energy_lane\w*\b", code)) == {"energy_lane"}
    assert len(re.findall(r"\bdouble\s+energy_lane\s*\(", code)) == 1
    assert len(re.findall(r"\bstruct\s+PTEns\b", code)) == 1
    assert "disorder_dev.h" in open(os.path.join(csrc, "build.sh")).read()

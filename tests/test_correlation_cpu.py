"""Correlation length without a GPU: the NumPy twin of the axis profiles and k_min modes (tests/helpers/correlation_twin.py) against
plain NumPy, the host-side summation of tsu.models.ising against the twin's restatement of the order, xi on synthetic series, the
exact chi(k_min) on a hand case, argument validation before any device call, and the C ABI's header / ctypes agreement."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_spec = importlib.util.spec_from_file_location("correlation_twin", os.path.join(HERE, "helpers", "correlation_twin.py"))
twin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(twin)

NEW_SYMBOLS = ["tsu_ising2d_profiles", "tsu_ising3d_profiles", "tsu_pt2d_set_correlation", "tsu_pt3d_set_correlation",
               "tsu_pt2d_history_modes", "tsu_pt3d_history_modes", "tsu_pt2d_profiles", "tsu_pt3d_profiles"]


def _spins(shape, seed):
    return np.where(np.random.default_rng(seed).integers(0, 2, size=shape) == 1, 1, -1).astype(np.int8)


@pytest.mark.parametrize("shape", [(6, 10), (33, 50), (3, 5, 18), (1, 8, 20)])
def test_twin_profiles_are_plain_sums(shape):
    a, b = _spins(shape, 1), _spins(shape, 2)
    for f, got in ((a.astype(np.int64), twin.profiles(a)), (a.astype(np.int64) * b, twin.profiles(a, b))):
        assert len(got) == len(shape)
        for d, P in enumerate(got):
            other = tuple(k for k in range(len(shape)) if k != d)
            assert P.dtype == np.int64
            np.testing.assert_array_equal(P, f.sum(axis=other))
            assert P.sum() == f.sum()


@pytest.mark.parametrize("shape", [(6, 10), (130, 272), (4, 16384), (4, 6, 34), (16, 16, 16)])
def test_twin_modes_agree_with_the_fft(shape):
    """F_d = conj(fft(P_d)[1]) (numpy's fft carries exp(-i ..)).  Tolerance 1e-9 N: at most 16384 terms of magnitude <= N, each
    product and add rounding by 2^-53 relative, gives <= 16384 * 2 * 1.1e-16 * N = 3.6e-12 N."""
    a, b = _spins(shape, 3), _spins(shape, 4)
    N = a.size
    for profs in (twin.profiles(a), twin.profiles(a, b)):
        got = twin.modes(profs, True)
        for d, P in enumerate(profs):
            want = np.conj(np.fft.fft(P.astype(np.float64))[1])
            assert abs(got[d] - want) <= 1e-9 * N, (d, got[d], want)
    half_open = twin.modes(twin.profiles(a), (True,) + (False,) * (len(shape) - 1))
    assert np.isfinite(half_open[0]) and np.all(np.isnan(half_open[1:]))


def test_host_summation_is_the_twins_order():
    """tsu.models.ising sums on the host (fourier_modes) in the vectorised form of the order the twin spells out term by term."""
    from tsu.models import ising
    rng = np.random.default_rng(5)
    for n in (1, 4, 63, 256, 257, 1000, 16400):
        terms = rng.normal(size=n) * 10.0 ** rng.integers(-3, 6, size=n)
        assert ising._ordered_sum(terms) == twin.ordered_sum(terms), n
    for L in (4, 6, 18, 272, 16400):
        for got, want in zip(ising._kmin_tables(L), twin.tables(L)):
            np.testing.assert_array_equal(got, want)
    profs = twin.profiles(_spins((12, 20), 6))
    np.testing.assert_array_equal(ising._kmin_modes(profs, (True, False))[:1], twin.modes(profs, (True, False))[:1])
    assert np.isnan(ising._kmin_modes(profs, (True, False))[1])


def test_xi_on_synthetic_series():
    from tsu.models import ising
    L = 16
    # <f^2> / <|F|^2> = 5 -> sqrt(4) / (2 sin(pi / 16))
    want = 2.0 / (2.0 * np.sin(np.pi / L))
    assert twin.xi(50.0, 10.0, L) == pytest.approx(want, rel=1e-15)
    assert np.isnan(twin.xi(5.0, 10.0, L))          # negative radicand
    assert twin.xi(10.0, 10.0, L) == 0.0
    got = ising.correlation_length([50.0, 5.0], [[10.0, np.nan], [10.0, 2.5]], (L, 8))
    assert got.shape == (2, 2)
    assert got[0, 0] == pytest.approx(want, rel=1e-15) and np.isnan(got[0, 1])
    assert np.isnan(got[1, 0]) and got[1, 1] == pytest.approx(1.0 / (2.0 * np.sin(np.pi / 8)), rel=1e-15)
    out = ising._correlation_summary({}, 128, (L, 8), (True, False), [50.0, 5.0], [[10.0, np.nan], [10.0, np.nan]])
    assert out["chi_k"].shape == out["xi"].shape == (2, 2) and out["xi_over_L"].shape == (2,)
    assert out["chi_k"][0, 0] == 10.0 / 128 and out["xi_over_L"][0] == pytest.approx(want / L) and np.isnan(out["xi_over_L"][1])


def test_exact_chi_k_on_a_2x2_hand_case():
    """Two uncoupled horizontal bonds of strength J: <s_i s_j> = tanh(J / T) =: t across a bond, 1 on the diagonal, 0 between the
    rows.  k = pi on both axes, so cos(k dx) = -1 across a bond along the column axis and +1 along the row axis:
    chi_col = 4 - 4 t^2, chi_row = 4 + 4 t^2.  Without couplings both are N = 4."""
    J, T = 0.7, 1.3
    jr = np.array([[J, 0.0], [J, 0.0]], np.float32)
    z = np.zeros((2, 2), np.float32)
    t = np.tanh(float(np.float32(J)) / T)
    got = twin.exact_chi_k((2, 2), True, (jr, z, None), T)
    np.testing.assert_allclose(got, [4 + 4 * t * t, 4 - 4 * t * t], rtol=1e-12)
    np.testing.assert_allclose(twin.exact_chi_k((2, 2), True, (z, z, None), T), [4.0, 4.0], rtol=1e-12)
    # a strong field aligns everything: <s_i s_j> -> 1 and the k = pi mode of a constant vanishes
    h = np.full((2, 2), 50.0, np.float32)
    np.testing.assert_allclose(twin.exact_chi_k((2, 2), True, (z, z, h), T), [0.0, 0.0], atol=1e-12)
    # 3-D form of the same problem, open z: no mode there
    got3 = twin.exact_chi_k((1, 2, 2), (False, True, True), (jr[None], z[None], z[None], None), T)
    assert np.isnan(got3[0])
    np.testing.assert_allclose(got3[1:], got, rtol=1e-12)


def test_no_periodic_axis_is_refused_before_any_device_call():
    from tsu.models import ising
    for call in (lambda: ising.temperature_scan(8, [2.0], periodic=False, correlation=True),
                 lambda: ising.temperature_scan_3d((4, 4, 4), [2.0], periodic=False, correlation=True),
                 lambda: ising.tempering_scan(8, [1.0, 2.0], periodic=False, correlation=True),
                 lambda: ising.tempering_scan_3d((4, 4, 4), [1.0, 2.0], periodic=(False, False, False), correlation=True),
                 lambda: ising.LatticeTempering(8, [1.0, 2.0], periodic=False, correlation=True),
                 lambda: ising.LatticeTempering3D((4, 4, 4), [1.0, 2.0], periodic=False, correlation=True)):
        with pytest.raises(ValueError, match="periodic axis"):
            call()


def test_shape_mismatch_and_table_validation_on_the_host():
    from tsu import _hip
    from tsu.models import ising
    a, b = ising.IsingModel2D.__new__(ising.IsingModel2D), ising.IsingModel2D.__new__(ising.IsingModel2D)
    a.rows, a.cols, b.rows, b.cols = 8, 16, 8, 12
    with pytest.raises(ValueError, match="equal shapes"):
        a.axis_profiles(b)
    a3, b3 = ising.IsingModel3D.__new__(ising.IsingModel3D), ising.IsingModel3D.__new__(ising.IsingModel3D)
    a3.shape, b3.shape = (4, 4, 8), (4, 8, 4)
    with pytest.raises(ValueError, match="equal shapes"):
        a3.fourier_modes(b3)
    pt = _hip.TemperingLattice.__new__(_hip.TemperingLattice)  # no handle: the checks below come before the C call
    pt.shape, pt.periodic = (8, 16), True
    with pytest.raises(ValueError, match="per axis"):
        pt.set_correlation(True, [twin.tables(8)])
    with pytest.raises(ValueError, match="length 16"):
        pt.set_correlation(True, [twin.tables(8), twin.tables(8)])
    pt.h = None  # nothing to destroy


def test_header_and_ctypes_prototypes_agree():
    """The entry points are declared in include/tsu_hip_correlation.h, which tsu_hip.h includes, exported by the library, and
    prototyped one to one in _hip.CORRELATION_SIGNATURES (which load_library declares)."""
    from tsu import _hip
    with open(os.path.join(ROOT, "include", "tsu_hip.h")) as f:
        assert re.search(r'^#include "tsu_hip_correlation.h"', f.read(), flags=re.M)
    with open(os.path.join(ROOT, "include", "tsu_hip_correlation.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tsu_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_hip.CORRELATION_SIGNATURES)
    lib = _hip.load_library()
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW_SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_hip.CORRELATION_SIGNATURES[name][1]), name
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == _hip.CORRELATION_SIGNATURES[name][1]
    for cls in (_hip.Lattice, _hip.Lattice3D, _hip.TemperingLattice, _hip.TemperingLattice3D):
        assert callable(getattr(cls, "profiles"))
    for cls in (_hip.TemperingLattice, _hip.TemperingLattice3D):
        assert callable(cls.set_correlation) and callable(cls.history_modes)


def test_python_surface():
    import inspect
    from tsu.models import ising
    for fn in (ising.temperature_scan, ising.temperature_scan_3d, ising.tempering_scan, ising.tempering_scan_3d,
               ising.LatticeTempering.__init__, ising.LatticeTempering3D.__init__):
        assert inspect.signature(fn).parameters["correlation"].default is False
    for cls in (ising.IsingModel2D, ising.IsingModel3D):
        assert callable(cls.axis_profiles) and callable(cls.fourier_modes)

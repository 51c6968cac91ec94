"""Overlaps of walker pairs without a GPU: the twin of the link overlap and of the family mask (tests/helpers/overlap_twin.py) against
identities and the energy twin's bond set, the host estimators of tsu.models.ising on synthetic records, the C ABI's header / ctypes
agreement, and argument validation before any device call."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


twin = _load("overlap_twin")
lattice3d_twin = _load("lattice3d_twin")

NEW_SYMBOLS = (["tsu_ising2d_link_overlap", "tsu_ising3d_link_overlap"]
               + [pre + name for pre in ("tsu_pt2d_", "tsu_pt3d_") for name in ("set_link_overlap", "history_link")]
               + [pre + name for pre in ("tsu_pa2d_", "tsu_pa3d_") for name in ("set_overlap", "history_overlap")])

SHAPES = [((5, 37), False), ((4, 4), True), ((6, 18), True), ((3, 4, 6), (False, True, True)), ((2, 3, 18), False),
          ((4, 4, 16), True), ((1, 6, 17), False), ((4, 2, 2), (True, False, False))]


def _spins(shape, seed):
    return (2 * np.random.default_rng(seed).integers(0, 2, size=shape) - 1).astype(np.int8)


# ---------------------------------------------------------------- header and bindings
def test_header_and_ctypes_prototypes_agree():
    """The entry points are declared in include/tsu_hip_overlap.h, which tsu_hip.h includes after tsu_hip_population.h, exported by
    the library, and prototyped one to one in _hip.OVERLAP_SIGNATURES (which load_library declares)."""
    from tsu import _hip
    with open(os.path.join(ROOT, "include", "tsu_hip.h")) as f:
        top = f.read()
    assert re.search(r'^#include "tsu_hip_overlap.h"', top, flags=re.M)
    assert top.index('#include "tsu_hip_population.h"') < top.index('#include "tsu_hip_overlap.h"')
    with open(os.path.join(ROOT, "include", "tsu_hip_overlap.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tsu_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_hip.OVERLAP_SIGNATURES)
    lib = _hip.load_library()
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW_SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_hip.OVERLAP_SIGNATURES[name][1]), name
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == _hip.OVERLAP_SIGNATURES[name][1]
    older = set(_hip.SIGNATURES) | set(_hip.CLUSTER3D_SIGNATURES) | set(_hip.CORRELATION_SIGNATURES) | set(_hip.POPULATION_SIGNATURES)
    assert not older & set(NEW_SYMBOLS)
    build = open(os.path.join(ROOT, "tsu-emulator_amd", "csrc", "build.sh")).read()
    for header_name in ("link_dev.h", "tsu_hip_overlap.h"):
        assert header_name in build, header_name


def test_python_surface():
    import inspect
    from tsu.models import ising
    for cls in (ising.IsingModel2D, ising.IsingModel3D):
        assert callable(cls.link_overlap)
    for cls in (ising.PopulationAnnealing, ising.PopulationAnnealing3D):
        assert callable(cls.overlap_stats) and callable(cls.overlap_histogram)
        p = inspect.signature(cls.__init__).parameters
        assert p["overlap"].default is False and p["correlation"].default is False
    for fn in (ising.population_annealing_scan, ising.population_annealing_scan_3d):
        p = inspect.signature(fn).parameters
        assert p["overlap"].default is False and p["correlation"].default is False
    for fn in (ising.LatticeTempering.__init__, ising.LatticeTempering3D.__init__, ising.tempering_scan, ising.tempering_scan_3d):
        assert inspect.signature(fn).parameters["link_overlap"].default is False


# ---------------------------------------------------------------- the twin against identities and the energy's bond set
@pytest.mark.parametrize("shape,periodic", SHAPES)
def test_twin_identities(shape, periodic):
    a, b = _spins(shape, 1), _spins(shape, 2)
    nb = twin.bond_count(shape, periodic)
    assert twin.link_overlap(a, a, periodic) == (nb, nb)
    assert twin.link_overlap(a, -a, periodic) == (nb, nb)
    L, n = twin.link_overlap(a, b, periodic)
    assert n == nb and abs(L) <= nb and (L - nb) % 2 == 0
    assert twin.link_overlap(b, a, periodic) == (L, nb)
    from tsu.models.ising import lattice_bond_count
    assert lattice_bond_count(shape, periodic) == nb


@pytest.mark.parametrize("shape,periodic", SHAPES)
def test_twin_one_flipped_site(shape, periodic):
    a = _spins(shape, 3)
    nb = twin.bond_count(shape, periodic)
    rng = np.random.default_rng(4)
    corners = [tuple(0 for _ in shape), tuple(n - 1 for n in shape)]
    for site in corners + [tuple(int(rng.integers(0, n)) for n in shape) for _ in range(6)]:
        b = a.copy()
        b[site] = -b[site]
        assert twin.link_overlap(a, b, periodic)[0] == nb - 2 * twin.degree(shape, periodic, site), site


@pytest.mark.parametrize("shape,periodic", [((3, 4, 6), False), ((3, 4, 6), True), ((3, 4, 6), (False, True, True)),
                                            ((4, 2, 2), (True, False, False)), ((1, 6, 17), False), ((2, 4, 4), (False, True, False))])
def test_twin_bond_set_is_the_energys(shape, periodic):
    """With J = 1 on every bond and no field, E of the all-up state is -N_b by the energy twin; and on random planes the energy twin
    evaluated on the overlap field p = a b gives -L."""
    one = np.ones(shape, np.float32)
    up = np.ones(shape, np.int8)
    E, terms = lattice3d_twin.energy_terms(up, periodic, one, one, one)
    assert -E == terms == twin.bond_count(shape, periodic)
    a, b = _spins(shape, 5), _spins(shape, 6)
    assert -lattice3d_twin.energy(a * b, periodic, one, one, one) == twin.link_overlap(a, b, periodic)[0]


def test_twin_short_periodic_axes_count_as_the_energy_does():
    """A periodic axis of length 2 bonds each pair twice and one of length 1 bonds each site to itself (np.roll in the energy twin)."""
    a, b = _spins((1, 2, 5), 7), _spins((1, 2, 5), 8)
    one = np.ones((1, 2, 5), np.float32)
    per = (True, True, False)
    assert twin.bond_count((1, 2, 5), per) == 10 + 10 + 8
    assert -lattice3d_twin.energy(a * b, per, one, one, one) == twin.link_overlap(a, b, per)[0]


# ---------------------------------------------------------------- pairing and the family mask
def test_pairs_and_family_mask_by_hand():
    assert twin.pairs(2) == [(0, 1)] and twin.pairs(5) == [(0, 2), (1, 3)] and twin.pairs(6) == [(0, 3), (1, 4), (2, 5)]
    # R = 6.  Step 1: walker 3 dies and takes a copy of 0 (pair 0 = (0, 3) falls into family 0).  Step 2: nothing.  Step 3: family 0
    # takes both halves: walkers 1, 2, 4, 5 copy 0 or 3.  Step 4: identity, the mask stays.
    parent = np.array([[0, 1, 2, 0, 4, 5],
                       [0, 1, 2, 3, 4, 5],
                       [0, 0, 3, 3, 0, 3],
                       [0, 1, 2, 3, 4, 5]])
    want = np.array([[True, True, True], [False, True, True], [False, True, True], [False, False, False], [False, False, False]])
    np.testing.assert_array_equal(twin.pair_mask(parent), want)
    from tsu.models.ising import population_pair_mask
    np.testing.assert_array_equal(population_pair_mask(parent), want)
    # odd R: the last walker has no partner, whatever it copies
    parent = np.array([[0, 1, 2, 3, 0], [1, 1, 2, 3, 4], [0, 1, 0, 3, 4]])
    want = np.array([[True, True], [True, True], [True, True], [False, True]])
    np.testing.assert_array_equal(twin.pair_mask(parent), want)
    np.testing.assert_array_equal(population_pair_mask(parent), want)
    rng = np.random.default_rng(9)
    parent = rng.integers(0, 40, size=(7, 40))
    np.testing.assert_array_equal(population_pair_mask(parent), twin.pair_mask(parent))


# ---------------------------------------------------------------- host estimators on a synthetic record
def test_overlap_stats_and_histogram_on_a_synthetic_record():
    from tsu.models import ising
    N, nb = 16, 32
    parent = np.array([[0, 1, 2, 0, 4, 5], [0, 0, 3, 3, 0, 3]])  # masks: TTT, FTT, FFF
    q = np.array([[16, -8, 4], [12, -16, 8], [2, 4, 6]], np.int64)
    ql = np.array([[32, 0, -8], [30, 16, -16], [1, 2, 3]], np.int64)
    modes = np.full((3, 3, 2), complex(np.nan, np.nan))
    modes[:, :, 1] = np.array([[3 + 4j, 1j, 2], [5, 6j, 8], [1, 1, 1]])
    out = ising.population_overlap_stats(parent, q, ql, N, nb, modes, (4, 4), (False, True))
    np.testing.assert_array_equal(out["pairs"], [3, 2, 0])
    Q0, Q1 = np.array([1.0, -0.5, 0.25]), np.array([-1.0, 0.5])
    np.testing.assert_allclose(out["overlap"][:2], [np.abs(Q0).mean(), np.abs(Q1).mean()], rtol=1e-15)
    np.testing.assert_allclose(out["overlap_sq"][:2], [(Q0 ** 2).mean(), (Q1 ** 2).mean()], rtol=1e-15)
    np.testing.assert_allclose(out["binder"][:2], [0.5 * (3 - (Q0 ** 4).mean() / (Q0 ** 2).mean() ** 2),
                                                   0.5 * (3 - (Q1 ** 4).mean() / (Q1 ** 2).mean() ** 2)], rtol=1e-15)
    np.testing.assert_allclose(out["link_overlap"][:2], [(32 + 0 - 8) / 3 / nb, (16 - 16) / 2 / nb], atol=1e-16)
    F2 = np.array([(25 + 1 + 4) / 3.0, (36 + 64) / 2.0])
    np.testing.assert_allclose(out["chi_k"][:2, 1], F2 / N, rtol=1e-15)
    assert np.isnan(out["chi_k"][:, 0]).all()
    want_xi = ising.correlation_length(out["overlap_sq"][:2] * N * N, np.stack([np.full(2, np.nan), F2], axis=1), (4, 4))
    np.testing.assert_array_equal(out["xi"][:2], want_xi)
    np.testing.assert_allclose(out["xi_over_L"][:2], want_xi[:, 1] / 4, rtol=1e-15)
    for key in ("overlap", "overlap_sq", "binder", "link_overlap", "xi_over_L"):
        assert np.isnan(out[key][2]), key  # no valid pair: NaN, not the numbers of the invalid ones
    assert np.isnan(out["chi_k"][2]).all() and np.isnan(out["xi"][2]).all()
    plain = ising.population_overlap_stats(parent, q, ql, N, nb)
    assert sorted(plain) == ["binder", "link_overlap", "overlap", "overlap_sq", "pairs"]
    h = ising.population_overlap_histogram(parent, q, N, bins=4)
    np.testing.assert_array_equal(h["edges"], [-1.0, -0.5, 0.0, 0.5, 1.0])
    np.testing.assert_array_equal(h["pairs"], [3, 2, 0])
    np.testing.assert_allclose(h["P"][0], np.array([0, 1, 1, 1]) / (3 * 0.5))  # -0.5 -> [-0.5, 0), 0.25, 1.0 (closed last bin)
    np.testing.assert_allclose(h["P"][1], np.array([1, 0, 0, 1]) / (2 * 0.5))
    assert np.isnan(h["P"][2]).all()
    assert h["P"][0].sum() * 0.5 == pytest.approx(1.0)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="bins"):
            ising.population_overlap_histogram(parent, q, N, bins=bad)


def test_the_record_joins_the_overlap_rows_of_split_runs():
    """PopulationAnnealing.run joins a later run's rows dropping its row 0 for the keys with n + 1 rows, q, q_link and modes included."""
    from tsu.models import ising

    class Handle:
        shape, step_count, calls = (4, 4), 0, 0

        def run(self, n, theta, resample, record):
            self.step_count += n
            self.n = n

        def history(self):
            n, base = self.n, 10 * self.calls
            self.calls += 1
            rows = lambda k, w: base + np.arange(k * w).reshape(k, w)  # noqa: E731
            return {"E": rows(n + 1, 4).astype(float), "M": rows(n + 1, 4), "W": rows(n, 4), "parent": np.tile(np.arange(4), (n, 1)),
                    "S": rows(n, 1)[:, 0], "U": rows(n, 1)[:, 0], "E_min": np.zeros(n), "resampled": np.full(n, True),
                    "q": rows(n + 1, 2), "q_link": rows(n + 1, 2), "modes": rows(n + 1, 2)[:, :, None] * (1 + 0j)}
    pa = ising.PopulationAnnealing.__new__(ising.PopulationAnnealing)
    pa.betas, pa.sweeps_per_step, pa._pa, pa.periodic = np.linspace(0.0, 1.0, 6), 1, Handle(), (False, True)
    pa.population, pa.n_spins, pa.overlap, pa.correlation = 4, 16, True, True
    pa._record, pa._complete = None, True
    pa.run(2)
    h = pa.run(3)
    assert h["q"].shape == (6, 2) and h["q_link"].shape == (6, 2) and h["modes"].shape == (6, 2, 2) and h["parent"].shape == (5, 4)
    assert np.isnan(h["modes"][:, :, 0]).all() and (h["modes"][3:, :, 1].real == h["q"][3:]).all()
    assert (h["q"][:3] == np.arange(6).reshape(3, 2)).all() and (h["q"][3:] == 10 + np.arange(2, 8).reshape(3, 2)).all()
    st = pa.overlap_stats()
    assert st["pairs"].tolist() == [2] * 6 and st["betas"].shape == (6,) and st["chi_k"].shape == (6, 2)
    assert pa.overlap_histogram(8)["P"].shape == (6, 8)


# ---------------------------------------------------------------- errors before any device call
def test_arguments_are_refused_before_any_device_call(monkeypatch):
    from tsu import _hip
    from tsu.models import ising

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_hip, "load_library", no_device)
    monkeypatch.setattr(_hip.Context, "default", classmethod(no_device))
    ok = dict(betas=[0.0, 0.5, 1.0])
    for make, size in ((ising.PopulationAnnealing, 8), (ising.PopulationAnnealing3D, (4, 4, 4))):
        with pytest.raises(ValueError, match="needs overlap=True"):
            make(size, 16, correlation=True, **ok)
        with pytest.raises(ValueError, match="periodic axis"):  # the error LatticeTempering(correlation=True) raises
            make(size, 16, overlap=True, correlation=True, periodic=False, **ok)
    for fn, size in ((ising.population_annealing_scan, 8), (ising.population_annealing_scan_3d, (4, 4, 4))):
        with pytest.raises(ValueError, match="needs overlap=True"):
            fn(size, 16, correlation=True, **ok)
    with pytest.raises(ValueError, match="ladders=2"):
        ising.LatticeTempering(8, [1.0, 2.0], link_overlap=True)
    with pytest.raises(ValueError, match="ladders=2"):
        ising.LatticeTempering3D((4, 4, 4), [1.0, 2.0], link_overlap=True)
    with pytest.raises(ValueError, match="replicas=2"):
        ising.tempering_scan(8, [1.0, 2.0], link_overlap=True)
    with pytest.raises(ValueError, match="replicas=2"):
        ising.tempering_scan_3d((4, 4, 4), [1.0, 2.0], link_overlap=True)


def test_estimators_need_the_overlap_record():
    from tsu.models import ising
    pa = ising.PopulationAnnealing.__new__(ising.PopulationAnnealing)
    pa._complete, pa._record = True, {"parent": np.zeros((1, 4), int), "E": np.zeros((2, 4))}
    for call in (pa.overlap_stats, pa.overlap_histogram):
        with pytest.raises(ValueError, match="overlap=True"):
            call()
    pa._record = None
    with pytest.raises(ValueError, match="every step"):
        pa.overlap_stats()

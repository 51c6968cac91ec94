"""K9's axis profiles and k_min modes on the host: the twin's positional count on packed words against its per-sample profiles,
the sum rule, the modes against the package's _kmin_modes, the Python layer's refusals before the device is touched, and the new
header and ctypes prototypes (no GPU needed)."""
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


twin = _load("multispin_corr_twin")
msc = twin.msc

# shape, periodic, S, replicas: pad bits (S = 3, 65), an open axis, a one-layer shape, one replica
CASES = [((4, 4, 6), True, 3, 2), ((4, 4, 6), True, 3, 1), ((4, 6, 8), (True, False, True), 65, 2), ((1, 8, 12), (False, True, True), 5, 2),
         ((6, 4, 18), True, 64, 2)]


def _random_planes(shape, S, A, R=2, seed=0):
    rng = np.random.default_rng(seed)
    W = (S + 63) // 64
    return rng.integers(0, 2 ** 63, size=(R, A, W) + shape, dtype=np.uint64) << np.uint64(1) | rng.integers(
        0, 2, size=(R, A, W) + shape, dtype=np.uint64)  # all 64 bits random, the pad bits too


@pytest.mark.parametrize("shape,periodic,S,A", CASES)
def test_packed_count_is_the_unpacked_one(shape, periodic, S, A):
    planes = _random_planes(shape, S, A, seed=S + A)
    want = twin.profiles(planes, S)
    got = twin.packed_profiles(planes, S)
    N = int(np.prod(shape))
    spins = twin.spins_of(planes, S).astype(np.int64)
    total = (spins[:, 0] * spins[:, 1] if A == 2 else spins[:, 0]).reshape(2, S, -1).sum(axis=2)  # q N, or sum s
    assert abs(total).max() <= N
    for d in range(3):
        assert got[d].shape == (2, S, shape[d]) and got[d].dtype == np.int64
        assert (got[d] == want[d]).all()
        assert (got[d].sum(axis=2) == total).all()
    # the pad columns are counted like any other and dropped at the end
    full = twin.packed_profiles(planes, S, with_pad=True)
    assert full[0].shape[1] == 64 * ((S + 63) // 64)
    if S % 64:
        everything = twin.profiles(planes, full[0].shape[1])
        assert all((f == e).all() for f, e in zip(full, everything))


def test_parts_and_the_counter_bound():
    """A coordinate of up to 64 * 255 sites is one part (a lane adds at most 255 words: 8 counter planes hold them); one site more
    makes two parts, each within the bound, and the shares still add up to the profile."""
    assert twin.parts_of(16320) == (1, 16320) and twin.parts_of(16321) == (2, 8161) and twin.parts_of(1) == (1, 1)
    for n in (16320, 16321, 40000):
        parts, chunk = twin.parts_of(n)
        assert chunk <= 64 * 255 and parts * chunk >= n and (parts - 1) * chunk < n
    rng = np.random.default_rng(1)
    ones = np.full(16320, ~np.uint64(0))
    assert (twin._part_counts(ones) == 16320).all()  # every lane's counter at 255 = 2^8 - 1
    with pytest.raises(AssertionError):
        twin._part_counts(np.full(16321, ~np.uint64(0)))
    words = rng.integers(0, 2 ** 63, size=16320, dtype=np.uint64)
    want = np.array([int(((words >> np.uint64(b)) & np.uint64(1)).sum()) for b in range(64)])
    assert (twin._part_counts(words) == want).all()
    # a one-layer plane with more sites than one part: P_z's single coordinate is cut in two
    shape, S = (1, 130, 126), 2
    planes = _random_planes(shape, S, 2, R=1, seed=9)
    assert twin.parts_of(130 * 126)[0] == 2
    assert all((g == w).all() for g, w in zip(twin.packed_profiles(planes, S), twin.profiles(planes, S)))


@pytest.mark.parametrize("shape,periodic,S,A", CASES + [((1, 4, 260), (False, True, True), 2, 2), ((1, 4, 516), (False, True, True), 2, 1)])
def test_modes_are_the_packages(shape, periodic, S, A):
    """correlation_twin.modes of the twin's profiles is tsu.models.ising._kmin_modes of them, bit for bit (axes longer than 256 wrap
    the 256 partials once and twice); NaN exactly on the open axes."""
    from tsu import _hip
    from tsu.models.ising import _kmin_modes
    per = _hip.periodic_axes(periodic)
    planes = _random_planes(shape, S, A, seed=7)
    profs = twin.packed_profiles(planes, S)
    got = twin.modes(profs, per)
    assert got.shape == (2, S, 3)
    for t in range(2):
        for s in range(S):
            assert twin.same_bits(got[t, s], _kmin_modes([P[t, s] for P in profs], per))
    for d in range(3):
        assert np.isnan(got[..., d]).all() == (not per[d]) and np.isnan(got[..., d]).any() == (not per[d])


NEW_SYMBOLS = ("tsu_msc_profiles", "tsu_msc_set_correlation", "tsu_msc_modes", "tsu_msc_pt_history_modes")


def test_header_and_ctypes_prototypes_agree():
    """The entry points are declared in include/tsu_hip_multispin_corr.h, which tsu_hip.h includes after tsu_hip_multispin_pt.h and
    build.sh lists, exported by the library and prototyped one to one in _hip.MULTISPIN_CORR_SIGNATURES (which load_library
    declares); the older headers and dicts hold none of them, and the package exports no new name."""
    from tsu import _hip
    with open(os.path.join(ROOT, "include", "tsu_hip.h")) as f:
        top = f.read()
    assert re.search(r'^#include "tsu_hip_multispin_corr.h"', top, flags=re.M)
    assert top.index('#include "tsu_hip_multispin_pt.h"') < top.index('#include "tsu_hip_multispin_corr.h"')
    with open(os.path.join(ROOT, "include", "tsu_hip_multispin_corr.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tsu_msc_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_hip.MULTISPIN_CORR_SIGNATURES)
    lib = _hip.load_library()
    for name in NEW_SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_hip.MULTISPIN_CORR_SIGNATURES[name][1]), name
        assert getattr(lib, name).argtypes == _hip.MULTISPIN_CORR_SIGNATURES[name][1]
    older = [_hip.SIGNATURES, _hip.CLUSTER3D_SIGNATURES, _hip.CORRELATION_SIGNATURES, _hip.POPULATION_SIGNATURES, _hip.OVERLAP_SIGNATURES,
             _hip.ENSEMBLE_SIGNATURES, _hip.SPARSE_BATCH_SIGNATURES, _hip.PROBE_SIGNATURES, _hip.CLUSTER_FIELD_SIGNATURES,
             _hip.MULTISPIN_SIGNATURES, _hip.MULTISPIN_PT_SIGNATURES]
    for d in older:
        assert not set(_hip.MULTISPIN_CORR_SIGNATURES) & set(d)
    assert lib.tsu_version() == 100
    for older_header in ("tsu_hip_multispin.h", "tsu_hip_multispin_pt.h"):
        with open(os.path.join(ROOT, "include", older_header)) as f:
            text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
        assert not set(re.findall(r"\b(tsu_msc_[a-z0-9_]+)\s*\(", text)) & set(NEW_SYMBOLS)
    with open(os.path.join(ROOT, "tsu-emulator_amd", "csrc", "build.sh")) as f:
        assert "tsu_hip_multispin_corr.h" in f.read()
    with open(os.path.join(ROOT, "__graft_entry__.py")) as f:
        assert "MULTISPIN_CORR_SIGNATURES" in f.read()
    import tsu
    from tsu import models
    for mod in (tsu, models):
        assert mod.__all__[-2:] == ["MultispinTempering3D", "multispin_tempering_scan_3d"]
    for method in ("profiles", "set_correlation", "modes", "pt_history_modes"):
        assert callable(getattr(_hip.MultispinLattice, method))
    for method in ("axis_profiles", "fourier_modes"):
        assert callable(getattr(models.MultispinGlass3D, method))


def test_philox_tags_are_unchanged_and_the_kernels_are_where_they_belong():
    csrc = os.path.join(ROOT, "tsu-emulator_amd", "csrc")
    with open(os.path.join(csrc, "tsu_common.h")) as f:
        common = f.read()
    assert sorted(int(v) for v in re.findall(r"TSU_TAG_[A-Z_]+\s*=\s*(\d+)", common)) == list(range(13))
    with open(os.path.join(csrc, "multispin_corr.hip")) as f:
        hip = re.sub(r"//[^\n]*", "", f.read())
    assert set(re.findall(r"__global__[^;{]*?\b(k9_\w+)\s*\(", hip)) == {"k9_profile", "k9_modes"}
    assert "TSU_TAG_" not in hip and "tsu_philox" not in hip  # no random numbers
    assert "contract(off)" in hip and not re.search(r"\b(cos|sin|sincos|__cosf|__sinf)\s*\(", hip)  # host tables, rounded products
    with open(os.path.join(csrc, "multispin_host.h")) as f:
        host = re.sub(r"//[^\n]*", "", f.read())
    assert "msc_corr_enqueue_row" in host and "__global__" not in host


def test_refusals_come_before_the_device(monkeypatch):
    from tsu import _hip
    from tsu.models import MultispinGlass3D, MultispinTempering3D, edwards_anderson_samples, multispin_scan_3d

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_hip, "MultispinLattice", no_device)
    shape, open_ = (4, 4, 6), (False, False, False)
    j = edwards_anderson_samples(shape, 3, kind="bimodal", seed=1, periodic=open_)
    for make in (MultispinGlass3D, MultispinTempering3D):
        with pytest.raises(ValueError, match="correlation=True needs at least one periodic axis"):
            make(shape, [1.0, 2.0], couplings=j, periodic=open_, correlation=True)
        with pytest.raises(AssertionError, match="the device was touched"):  # without it the same arguments reach the handle
            make(shape, [1.0, 2.0], couplings=j, periodic=open_)
    with pytest.raises(ValueError, match="correlation=True needs at least one periodic axis"):
        multispin_scan_3d(shape, [1.0, 2.0], couplings=j, periodic=open_, correlation=True, n_equilibrate=0, n_measure=1)
    jp = edwards_anderson_samples(shape, 3, kind="bimodal", seed=1)
    with pytest.raises(AssertionError, match="the device was touched"):
        MultispinGlass3D(shape, [1.0, 2.0], couplings=jp, correlation=True)


def test_fourier_modes_needs_correlation():
    """With correlation off fourier_modes() raises, and neither the constructor nor it calls a new handle method."""
    from tsu import _hip
    from tsu.models import MultispinGlass3D, edwards_anderson_samples

    calls = []

    class Handle:
        def __init__(self, *a, **k):
            pass

        def __getattr__(self, name):
            calls.append(name)
            return lambda *a, **k: None

    shape = (4, 4, 6)
    j = edwards_anderson_samples(shape, 3, kind="bimodal", seed=1)
    orig = _hip.MultispinLattice
    _hip.MultispinLattice = Handle
    try:
        g = MultispinGlass3D(shape, [1.0, 2.0], couplings=j, replicas=2, seed=1)
        with pytest.raises(ValueError, match="fourier_modes needs correlation=True"):
            g.fourier_modes()
        assert not {"profiles", "set_correlation", "modes", "pt_history_modes"} & set(calls)
        calls.clear()
        mixed = (True, False, True)
        on = MultispinGlass3D(shape, [1.0, 2.0], couplings=edwards_anderson_samples(shape, 3, kind="bimodal", seed=1, periodic=mixed),
                              replicas=2, seed=1, correlation=True, periodic=mixed)
        assert calls.count("set_correlation") == 1 and on.correlation
    finally:
        _hip.MultispinLattice = orig

"""K9's real-space correlations, two-time correlations and quench runs on the host: the twin against a brute-force loop and the
sum rule, the kernel's plan and staging (packed words) against the twin, the xi_12 estimator against its plain-loop restatement,
the new header and ctypes prototypes, and the Python layer's refusals before the device is touched (no GPU needed)."""
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


twin = _load("multispin_quench_twin")
ALL = (True, True, True)


def _random_spins(shape, S, A, R=2, seed=0):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([-1, 1], np.int8), size=(R, A, S) + tuple(shape))


def _random_planes(shape, W, A, R=2, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2 ** 63, size=(R, A, W) + tuple(shape), dtype=np.uint64) << np.uint64(1) | rng.integers(
        0, 2, size=(R, A, W) + tuple(shape), dtype=np.uint64)  # all 64 bits random, the pad bits too


@pytest.mark.parametrize("A", [1, 2])
def test_twin_equals_the_triple_loop(A):
    shape, S = (2, 4, 6), 3
    s = _random_spins(shape, S, A, seed=A)
    got = twin.c4_twin(s, ALL)
    for t in range(2):
        for k in range(S):
            f = (s[t, 0, k].astype(int) * s[t, 1, k]) if A == 2 else s[t, 0, k].astype(int)
            for d in range(3):
                L = shape[d]
                assert got[d].shape == (2, S, L // 2 + 1) and got[d].dtype == np.int64
                for r in range(L // 2 + 1):
                    total = 0
                    for z in range(shape[0]):
                        for y in range(shape[1]):
                            for x in range(shape[2]):
                                at = [z, y, x]
                                at[d] = (at[d] + r) % L
                                total += f[z, y, x] * f[tuple(at)]
                    assert got[d][t, k, r] == total
    assert all((c[..., 0] == 2 * 4 * 6).all() for c in got)
    mixed = twin.c4_twin(s, (False, True, False))
    assert mixed[0] is None and mixed[2] is None and (mixed[1] == got[1]).all()


@pytest.mark.parametrize("shape", [(2, 4, 6), (4, 6, 8)])
def test_sum_rule(shape):
    """C[0] + 2 sum_{0 < r < L / 2} C[r] + C[L / 2] = sum over the axis's lines of (sum_x f_x)^2: every ordered pair of a line once."""
    s = _random_spins(shape, 5, 2, seed=3)
    f = s[:, 0].astype(np.int64) * s[:, 1]
    for d, c in enumerate(twin.c4_twin(s, ALL)):
        lines = (f.sum(axis=2 + d) ** 2).sum(axis=(2, 3))
        assert (c[..., 0] + 2 * c[..., 1:-1].sum(axis=-1) + c[..., -1] == lines).all()


def test_two_time_twin():
    now, snap = _random_spins((2, 4, 6), 3, 2, seed=5), _random_spins((2, 4, 6), 3, 2, seed=6)
    got = twin.two_time_twin(now, snap)
    assert got.shape == (2, 2, 3) and (twin.two_time_twin(now, now) == 48).all() and (twin.two_time_twin(now, -now) == -48).all()
    assert got[1, 0, 2] == sum(int(a) * int(b) for a, b in zip(now[1, 0, 2].ravel(), snap[1, 0, 2].ravel()))


# the GPU file's shapes, plus a row axis too long for 16-column slabs (1030 + 1 words x 16 > 16384: slabs of 8 columns)
PACKED = [((4, 4, 4), ALL, 2), ((1, 6, 20), (False, True, True), 2), ((4, 6, 36), (True, False, True), 1), ((4, 4, 136), ALL, 2),
          ((4, 4, 520), ALL, 2), ((4, 1030, 12), (False, True, False), 2)]


@pytest.mark.parametrize("shape,periodic,A", PACKED)
def test_packed_count_is_the_unpacked_one(shape, periodic, A):
    """The kernel's plan, staging maps and per-line counts on packed words (twin.packed_c4; it also asserts that every site lands
    in exactly one line of one bundle) give the roll products of the unpacked spins, pad bits included."""
    msc = _load("multispin_twin")
    planes = _random_planes(shape, 1, A, R=1, seed=sum(shape))
    spins = np.stack([np.stack([np.where(msc.unpack(planes[t, a], 64), 1, -1).astype(np.int8) for a in range(A)]) for t in range(1)])
    want = twin.c4_twin(spins, periodic)
    got = twin.packed_c4(planes, periodic)
    for d in range(3):
        assert (got[d] is None) == (not periodic[d]) == (want[d] is None)
        if periodic[d]:
            assert got[d].shape == (1, 64, shape[d] // 2 + 1) and (got[d] == want[d]).all()


def test_plan_limits():
    """A bundle never exceeds the LDS, a slab narrows only where 16 columns of the axis would, and the bundles cover the units."""
    for shape, periodic in [((4, 4, 4), ALL), ((64, 64, 64), ALL), ((4, 1022, 32), ALL), ((4, 1024, 32), ALL), ((4, 4, 16382), ALL),
                            ((16382, 1, 1), (True, False, False)), ((4, 6, 2), (True, True, False))]:
        for d, a in twin.c4_plan(shape, periodic).items():
            assert a["lds"] <= 144 * 1024 and a["nb"] * a["per"] >= a["nunits"] > (a["nb"] - 1) * a["per"]
            assert a["G"] * a["npw"] <= 64 and a["npw"] >= 1
            if d < 2:
                assert a["sw"] == min(16, max(1, 1 << (shape[2] - 1).bit_length())) or a["sw"] * 2 * (a["L"] + 1) > 16384
    assert twin.c4_plan((4, 1022, 32), ALL)[1]["sw"] == 16 and twin.c4_plan((4, 1024, 32), ALL)[1]["sw"] == 8
    with pytest.raises(AssertionError):
        twin.c4_plan((4, 4, 16384), ALL)


def test_xi12_estimator_against_the_twin():
    from tsu.models.ising import _xi12
    rng = np.random.default_rng(11)
    r = np.arange(9)
    # r_cut inside the range: the signal falls below 3 errors at some r; never: tiny noise on a slow decay
    inside = np.exp(-r / 1.5) + 0.02 * rng.normal(size=(12, 9))
    never = np.exp(-r / 6.0) + 1e-6 * rng.normal(size=(12, 9))
    inside[:, 0] = never[:, 0] = 1.0
    cuts = []
    for c4 in (inside, never, inside[:1]):
        mean, err, xi, xi_err, r_cut = _xi12(c4)
        want = twin.xi12_twin(c4)
        cuts.append(int(r_cut))
        assert int(r_cut) == want[2]
        assert xi == pytest.approx(want[0], rel=1e-12)
        if c4.shape[0] > 1:
            assert xi_err == pytest.approx(want[1], rel=1e-9) and xi_err > 0
            assert mean == pytest.approx(c4.mean(axis=0)) and err == pytest.approx(c4.std(axis=0, ddof=1) / np.sqrt(12))
        else:
            assert np.isnan(xi_err) and np.isnan(want[1]) and np.isnan(err).all()
    assert 0 < cuts[0] < 8 and cuts[1] == 8 and cuts[2] == 8
    # leading axes are carried along: (n_times, n_temps, S, R)
    both = np.stack([np.stack([inside, never]), np.stack([never, inside])])
    mean, err, xi, xi_err, r_cut = _xi12(both)
    assert xi.shape == (2, 2) and (r_cut == [[cuts[0], 8], [8, cuts[0]]]).all()
    assert xi[0, 1] == pytest.approx(twin.xi12_twin(never)[0], rel=1e-12) and xi_err[1, 1] == pytest.approx(twin.xi12_twin(inside)[1], rel=1e-9)
    assert twin.xi12_twin(inside, cut=0.0)[2] == 8 and int(_xi12(inside, cut=0.0)[4]) == 8


NEW_SYMBOLS = ("tsu_msc_c4", "tsu_msc_snapshot_slots", "tsu_msc_snapshot", "tsu_msc_snapshot_overlap", "tsu_msc_quench_run",
               "tsu_msc_quench_history")


def test_header_and_ctypes_prototypes_agree():
    """The entry points are declared in include/tsu_hip_multispin_quench.h, which tsu_hip.h includes after tsu_hip_multispin_corr.h
    and build.sh lists, exported by the library and prototyped one to one in _hip.MULTISPIN_QUENCH_SIGNATURES (which load_library
    declares and build() checks); the older headers and dicts hold none of them; the package exports one new name, ahead of the tail."""
    from tsu import _hip
    with open(os.path.join(ROOT, "include", "tsu_hip.h")) as f:
        top = f.read()
    assert re.search(r'^#include "tsu_hip_multispin_quench.h"', top, flags=re.M)
    assert top.index('#include "tsu_hip_multispin_corr.h"') < top.index('#include "tsu_hip_multispin_quench.h"')
    with open(os.path.join(ROOT, "include", "tsu_hip_multispin_quench.h")) as f:
        raw = f.read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(tsu_msc_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_hip.MULTISPIN_QUENCH_SIGNATURES)
    lib = _hip.load_library()
    for name in NEW_SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_hip.MULTISPIN_QUENCH_SIGNATURES[name][1]), name
        assert getattr(lib, name).argtypes == _hip.MULTISPIN_QUENCH_SIGNATURES[name][1]
    assert int(re.search(r"#define TSU_MSC_SNAPSHOT_SLOTS (\d+)", raw).group(1)) == _hip.MSC_SNAPSHOT_SLOTS == 8
    assert int(re.search(r"#define TSU_MSC_C4_MAX_AXIS (\d+)", raw).group(1)) == _hip.MSC_C4_MAX_AXIS == twin.MAX_AXIS
    older = [_hip.SIGNATURES, _hip.CLUSTER3D_SIGNATURES, _hip.CORRELATION_SIGNATURES, _hip.POPULATION_SIGNATURES, _hip.OVERLAP_SIGNATURES,
             _hip.ENSEMBLE_SIGNATURES, _hip.SPARSE_BATCH_SIGNATURES, _hip.PROBE_SIGNATURES, _hip.CLUSTER_FIELD_SIGNATURES,
             _hip.MULTISPIN_SIGNATURES, _hip.MULTISPIN_PT_SIGNATURES, _hip.MULTISPIN_CORR_SIGNATURES]
    for d in older:
        assert not set(_hip.MULTISPIN_QUENCH_SIGNATURES) & set(d)
    assert lib.tsu_version() == 100
    for older_header in ("tsu_hip_multispin.h", "tsu_hip_multispin_pt.h", "tsu_hip_multispin_corr.h"):
        with open(os.path.join(ROOT, "include", older_header)) as f:
            text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
        assert not set(re.findall(r"\b(tsu_msc_[a-z0-9_]+)\s*\(", text)) & set(NEW_SYMBOLS)
    with open(os.path.join(ROOT, "tsu-emulator_amd", "csrc", "build.sh")) as f:
        assert "tsu_hip_multispin_quench.h" in f.read()
    with open(os.path.join(ROOT, "__graft_entry__.py")) as f:
        assert "MULTISPIN_QUENCH_SIGNATURES" in f.read()
    import tsu
    from tsu import models
    for mod in (tsu, models):
        assert mod.__all__[-3:] == ["multispin_quench_3d", "MultispinTempering3D", "multispin_tempering_scan_3d"]
        assert callable(mod.multispin_quench_3d)
    for method in ("c4", "snapshot_slots", "snapshot", "snapshot_overlap", "quench_run", "quench_history"):
        assert callable(getattr(_hip.MultispinLattice, method))
    for method in ("overlap_correlation", "snapshot", "two_time", "quench"):
        assert callable(getattr(models.MultispinGlass3D, method)) and callable(getattr(models.MultispinTempering3D, method))


def test_the_kernels_are_where_they_belong():
    csrc = os.path.join(ROOT, "tsu-emulator_amd", "csrc")
    with open(os.path.join(csrc, "tsu_common.h")) as f:
        common = f.read()
    assert sorted(int(v) for v in re.findall(r"TSU_TAG_[A-Z_]+\s*=\s*(\d+)", common)) == list(range(13))  # no new Philox tag
    with open(os.path.join(csrc, "multispin_quench.hip")) as f:
        hip = f.read()
    assert "tsu_philox" not in hip and "TSU_TAG_" not in hip  # no random numbers
    code = re.sub(r"//[^\n]*", "", hip)
    assert set(re.findall(r"__global__[^;{]*?\b(k9_\w+)\s*\(", code)) == {"k9_c4", "k9_twotime"}
    assert not re.search(r"\b(float|double)\b", code)  # integers only
    with open(os.path.join(csrc, "multispin_host.h")) as f:
        host = re.sub(r"//[^\n]*", "", f.read())
    assert "msc_quench* qn;" in host and "msc_quench_free" in host and "__global__" not in host
    with open(os.path.join(csrc, "multispin.hip")) as f:
        assert "msc_quench_free(h);" in f.read()


class _Handle:
    """Stands in for _hip.MultispinLattice: records the methods the model calls."""
    calls = []

    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        _Handle.calls.append(name)
        return lambda *a, **k: None


def test_refusals_come_before_the_device(monkeypatch):
    from tsu import _hip
    from tsu.models import MultispinGlass3D, MultispinTempering3D, edwards_anderson_samples, multispin_quench_3d

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    shape, open_ = (4, 4, 6), (False, False, False)
    j = edwards_anderson_samples(shape, 3, kind="bimodal", seed=1)
    jo = edwards_anderson_samples(shape, 3, kind="bimodal", seed=1, periodic=open_)
    bad = [
        (dict(times=[]), "non-empty"),
        (dict(times=[[0, 1]]), "non-empty 1-D"),
        (dict(times=[0, 1.5]), "integer sweep counts"),
        (dict(times=[-1, 2]), "strictly ascending"),
        (dict(times=[0, 2, 2]), "strictly ascending"),
        (dict(times=[0, 3, 2]), "strictly ascending"),
        (dict(times=[0, 1, 2], waiting_times=[3]), "subset of times"),
        (dict(times=[0, 1, 2], waiting_times=[2, 1]), "waiting_times must be strictly ascending"),
        (dict(times=list(range(10)), waiting_times=list(range(9))), "at most 8 waiting_times"),
    ]
    monkeypatch.setattr(_hip, "MultispinLattice", no_device)
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            multispin_quench_3d(shape, [1.0, 2.0], couplings=j, **kw)
    with pytest.raises(ValueError, match="at least one periodic axis"):
        multispin_quench_3d(shape, [1.0, 2.0], couplings=jo, periodic=open_, times=[0, 1])
    with pytest.raises(ValueError, match="replicas must be 1 or 2"):
        multispin_quench_3d(shape, [1.0, 2.0], couplings=j, times=[0, 1], replicas=3)
    with pytest.raises(AssertionError, match="the device was touched"):  # good arguments reach the handle
        multispin_quench_3d(shape, [1.0, 2.0], couplings=j, times=[0, 1, 4], waiting_times=[1])
    # the methods of a model that exists: nothing reaches its handle
    monkeypatch.setattr(_hip, "MultispinLattice", _Handle)
    for make in (MultispinGlass3D, MultispinTempering3D):
        g = make(shape, [1.0, 2.0], couplings=j, replicas=2, seed=1)
        go = make(shape, [1.0, 2.0], couplings=jo, periodic=open_, replicas=2, seed=1)
        _Handle.calls.clear()
        for kw, match in bad:
            with pytest.raises(ValueError, match=match):
                g.quench(**kw)
        with pytest.raises(ValueError, match="at least one periodic axis"):
            go.quench([0, 1])
        with pytest.raises(ValueError, match="at least one periodic axis"):
            go.overlap_correlation()
        with pytest.raises(ValueError, match="slot 8 outside 0 .. 7"):
            g.snapshot(8)
        with pytest.raises(ValueError, match="slot 0 holds no snapshot"):
            g.two_time(0)
        g.sweep_count = (1 << 31) - 3
        with pytest.raises(ValueError, match="sweep counter overflow"):
            g.quench([0, 4])
        assert _Handle.calls == [] and g.sweep_count == (1 << 31) - 3
        g.sweep_count = 0
        g.snapshot(2)
        g.snapshot(1)
        assert _Handle.calls == ["snapshot_slots", "snapshot", "snapshot"]  # the slots grow once, to the highest asked for

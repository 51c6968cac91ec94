"""K9, multispin coding of the +-J glass, on the host: packing, the 13-entry threshold table, the bit-sliced update and counters
stated in NumPy against the per-sample twin, the Python layer's refusals before the device is touched, and the new header and
ctypes prototypes (no GPU needed)."""
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


twin = _load("multispin_twin")
lat3 = twin.lat3


@pytest.mark.parametrize("S", [1, 64, 65, 130])
def test_pack_unpack_round_trip(S):
    from tsu import _hip
    rng = np.random.default_rng(S)
    bits = rng.integers(0, 2, size=(S, 2, 3, 5)).astype(bool)
    for pack, unpack in ((twin.pack, twin.unpack), (_hip.msc_pack, _hip.msc_unpack)):
        w = pack(bits)
        assert w.dtype == np.uint64 and w.shape == ((S + 63) // 64, 2, 3, 5)
        assert (unpack(w, S) == bits).all()
    assert (twin.pack(bits) == _hip.msc_pack(bits)).all()
    w = twin.pack(bits)
    # bit b of word-plane w is sample 64 w + b; the pad bits are 0
    s = S - 1
    assert (((w[s // 64] >> np.uint64(s % 64)) & np.uint64(1)).astype(bool) == bits[s]).all()
    if S % 64:
        assert not np.any(w[-1] >> np.uint64(S % 64))


@pytest.mark.parametrize("T", [0.5, 1.1, 2.0, 4.5115])
def test_threshold_table_is_the_twins(T):
    from tsu import _hip
    t = _hip.msc_thresholds(T)
    want = lat3.thresholds(np.arange(-6, 7, dtype=np.float64), T)
    assert t.dtype == np.uint64 and t.shape == (13,)
    assert (t == want).all() and (t == twin.table(T)).all()
    assert (np.diff(t.astype(object)) >= 0).all()
    assert int(t[6]) == 2 ** 31
    if T == 0.5:  # f = +-6 sits beyond the +-20 clamp
        assert int(t[0]) == 0 and int(t[12]) == 2 ** 32
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="Temperature must be positive"):
            _hip.msc_thresholds(bad)


def _open_case(S=65, shape=(3, 5, 18), seed=5):
    from tsu.models import edwards_anderson_samples
    j = edwards_anderson_samples(shape, S, kind="bimodal", seed=seed, periodic=False)
    rng = np.random.default_rng(seed + 1)
    spins = rng.choice(np.array([-1, 1], np.int8), size=(S,) + shape)
    return j, spins


def test_bitsliced_update_is_the_per_sample_twin():
    """(3, 5, 18) all open, 65 samples, 3 sweeps: odd neighbour counts, a partial octet, a partial word."""
    shape, S, T, seed = (3, 5, 18), 65, 1.1, (7 << 32) | 12
    j, spins = _open_case(S, shape)
    packed = [twin.pack(a == -1) for a in j]
    got = twin.bitsliced_sweep(twin.pack(spins == 1), False, *packed, T, 3, seed)
    want = twin.reference_sweep(spins, False, j, T, 3, seed)
    assert (np.where(twin.unpack(got, S), 1, -1) == want).all()
    # sweep0 continues the same chain
    a = twin.bitsliced_sweep(twin.bitsliced_sweep(twin.pack(spins == 1), False, *packed, T, 1, seed), False, *packed, T, 2, seed, sweep0=1)
    assert (a == got).all()
    # the pad bits were swept like any other: they carry J = +1 and their own (all -1) start
    pad = lat3.sweep(np.full(shape, -1, np.int8), False, *lat3.uniform_disorder(shape, False, 1.0)[:3], None, T, 3, seed)
    assert (np.where((got[1] >> np.uint64(5)) & np.uint64(1), 1, -1) == pad).all()


def test_bitsliced_update_periodic_and_mixed():
    from tsu.models import edwards_anderson_samples
    for shape, periodic, T in (((4, 4, 4), True, 0.5), ((4, 6, 8), (True, False, True), 2.0)):
        S, seed = 3, 99
        j = edwards_anderson_samples(shape, S, kind="bimodal", seed=2, periodic=periodic)
        spins = np.random.default_rng(4).choice(np.array([-1, 1], np.int8), size=(S,) + shape)
        got = twin.bitsliced_sweep(twin.pack(spins == 1), periodic, *[twin.pack(a == -1) for a in j], T, 3, seed, sweep0=2)
        assert (np.where(twin.unpack(got, S), 1, -1) == twin.reference_sweep(spins, periodic, j, T, 3, seed, sweep0=2)).all()


def test_ties_take_the_low_half():
    """T = 2 f / logit(u / 2^32) of a colour-0 site puts its first decision on the threshold: the bit-sliced statement sees the tie
    and still agrees with the per-sample twin."""
    shape, S, seed = (4, 4, 4), 1, 3
    from tsu.models import edwards_anderson_samples
    j = edwards_anderson_samples(shape, S, kind="bimodal", seed=1)
    spins = np.ones((S,) + shape, np.int8)
    f = lat3.local_field(spins[0], True, *lat3.as_disorder(shape, j[0][0], j[1][0], j[2][0]))
    u = lat3.site_uniforms(shape, 0, seed).astype(np.float64) / 4294967296.0
    logit = np.log(u) - np.log1p(-u)
    ok = (lat3.colours(shape) == 0) & (f != 0) & (f * logit > 0)
    z, r, c = np.argwhere(ok)[0]
    T = float(2.0 * f[z, r, c] / logit[z, r, c])
    stats = {}
    got = twin.bitsliced_sweep(twin.pack(spins == 1), True, *[twin.pack(a == -1) for a in j], T, 2, seed, stats=stats)
    assert stats["ties"] >= 1 and twin.sample_ties(spins, True, j, T, 2, seed) >= 1
    assert (np.where(twin.unpack(got, S), 1, -1) == twin.reference_sweep(spins, True, j, T, 2, seed)).all()


def test_vertical_counters_equal_direct_sums():
    rng = np.random.default_rng(8)
    words = rng.integers(0, 2 ** 64, size=(100, 7), dtype=np.uint64)
    planes = [np.zeros(7, np.uint64) for _ in range(8)]
    for x in words:
        planes = twin.counters_add(planes, x)
    direct = np.stack([((words >> np.uint64(b)) & np.uint64(1)).astype(np.int64).sum(axis=0) for b in range(64)])
    assert (twin.counters_values(planes) == direct).all()
    # the adder of the update: six words into three count planes
    xs = [rng.integers(0, 2 ** 64, size=11, dtype=np.uint64) for _ in range(6)]
    b0, b1, b2 = twin.adder(xs)
    count = sum(((x[None] >> np.arange(64, dtype=np.uint64)[:, None]) & np.uint64(1)).astype(np.int64) for x in xs)
    assert (twin.counters_values([b0, b1, b2]) == count).all()
    # count >= k* for every k*
    for ks in range(9):
        got = twin.at_least(b0[None], b1[None], b2[None], np.full(11, ks))[0]
        assert (twin.counters_values([got])[:, :] == (count >= ks)).all(), ks


def test_unsatisfied_bonds_give_the_energy():
    """E = 2 unsat - N_b and q_l N_b = N_b - 2 count(a_i a_j b_i b_j = -1), from words."""
    from tsu.models.ising import lattice_bond_count
    shape, S = (3, 5, 18), 65
    j, a = _open_case(S, shape)
    b = np.random.default_rng(77).choice(np.array([-1, 1], np.int8), size=a.shape)
    wa, wb = twin.pack(a == 1), twin.pack(b == 1)
    packed = [twin.pack(x == -1) for x in j]
    nb = lattice_bond_count(shape, False)
    unsat = np.zeros(S, np.int64)
    differ = np.zeros(S, np.int64)
    for axis, J in ((2, packed[0]), (1, packed[1]), (0, packed[2])):
        keep = [slice(None)] * 4
        keep[axis + 1] = slice(0, shape[axis] - 1)  # an open axis lacks its last bond
        da, db = wa ^ np.roll(wa, -1, axis=axis + 1), wb ^ np.roll(wb, -1, axis=axis + 1)
        unsat += twin.unpack((da ^ J)[tuple(keep)], S).reshape(S, -1).sum(axis=1)
        differ += twin.unpack((da ^ db)[tuple(keep)], S).reshape(S, -1).sum(axis=1)
    assert (2 * unsat - nb == twin.reference_energy(a, False, j)).all()
    pa, pb = a.astype(np.int64), b.astype(np.int64)
    link = sum((pa * pb * np.roll(pa * pb, -1, axis=ax + 1))[tuple(slice(None) if k != ax + 1 else slice(0, shape[ax] - 1) for k in range(4))]
               .reshape(S, -1).sum(axis=1) for ax in range(3))
    assert (nb - 2 * differ == link).all()


def test_refusals_come_before_the_device(monkeypatch):
    from tsu import _hip
    from tsu.models import MultispinGlass3D, edwards_anderson_samples, multispin_scan_3d

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_hip, "MultispinLattice", no_device)
    shape = (4, 4, 6)
    j = edwards_anderson_samples(shape, 3, kind="bimodal", seed=1)
    with pytest.raises(ValueError, match=r"J_down.*\+-1 only.*0\.5"):
        bad = [a.copy() for a in j]
        bad[1][2, 1, 1, 1] = 0.5
        MultispinGlass3D(shape, [1.0], couplings=bad)
    with pytest.raises(ValueError, match="J_right.*Gaussian"):
        MultispinGlass3D(shape, [1.0], couplings=edwards_anderson_samples(shape, 3, kind="gaussian", seed=1))
    with pytest.raises(ValueError, match="J_layer.*0"):  # a diluted bond
        bad = [a.copy() for a in j]
        bad[2][0, 0, 0, 0] = 0.0
        MultispinGlass3D(shape, [1.0], couplings=bad)
    with pytest.raises(ValueError, match="field"):
        MultispinGlass3D(shape, [1.0], couplings=j, field=np.zeros(shape))
    with pytest.raises(ValueError, match=r"periodic axis.*rows = 5"):
        MultispinGlass3D((4, 5, 6), [1.0], couplings=edwards_anderson_samples((4, 5, 6), 3, seed=1))
    with pytest.raises(ValueError, match=r"periodic axis.*depth = 2"):
        MultispinGlass3D((2, 4, 6), [1.0], couplings=edwards_anderson_samples((2, 4, 6), 3, seed=1))
    # an open axis demands the zeros of its last slice, and nothing else there
    jo = edwards_anderson_samples(shape, 3, seed=1, periodic=(True, False, True))
    with pytest.raises(ValueError, match="J_down.*open rows axis"):
        MultispinGlass3D(shape, [1.0], couplings=j, periodic=(True, False, True))
    with pytest.raises(ValueError, match="shape"):
        MultispinGlass3D((4, 4, 8), [1.0], couplings=j)
    with pytest.raises(ValueError, match="Temperature must be positive"):
        MultispinGlass3D(shape, [1.0, 0.0], couplings=j)
    with pytest.raises(ValueError, match="replicas"):
        MultispinGlass3D(shape, [1.0], couplings=j, replicas=3)
    with pytest.raises(ValueError, match="route"):
        MultispinGlass3D(shape, [1.0], couplings=j, route="lds")
    with pytest.raises(ValueError, match="replicas"):
        multispin_scan_3d(shape, [1.0], couplings=j, replicas=0)
    # valid input reaches the handle
    for kw in (dict(couplings=j), dict(couplings=jo, periodic=(True, False, True))):
        with pytest.raises(AssertionError, match="the device was touched"):
            MultispinGlass3D(shape, [1.0, 2.0], replicas=2, seed=1, **kw)
    j2 = edwards_anderson_samples((6, 34), 64, dims=2, seed=3)
    with pytest.raises(AssertionError, match="the device was touched"):
        MultispinGlass3D((1, 6, 34), [1.5], couplings=j2, periodic=(False, True, True), seed=1)


NEW_SYMBOLS = ("tsu_msc_thresholds", "tsu_msc_create", "tsu_msc_destroy", "tsu_msc_route", "tsu_msc_set_couplings", "tsu_msc_set_planes",
               "tsu_msc_get_planes", "tsu_msc_set_seeds", "tsu_msc_randomize", "tsu_msc_fill", "tsu_msc_set_temperatures", "tsu_msc_sweep",
               "tsu_msc_measure", "tsu_msc_launch_count")


def test_header_and_ctypes_prototypes_agree():
    """The entry points are declared in include/tsu_hip_multispin.h, which tsu_hip.h includes after tsu_hip_cluster_field.h and build.sh
    lists, exported by the library and prototyped one to one in _hip.MULTISPIN_SIGNATURES (which load_library declares)."""
    from tsu import _hip
    with open(os.path.join(ROOT, "include", "tsu_hip.h")) as f:
        top = f.read()
    assert re.search(r'^#include "tsu_hip_multispin.h"', top, flags=re.M)
    assert top.index('#include "tsu_hip_cluster_field.h"') < top.index('#include "tsu_hip_multispin.h"')
    with open(os.path.join(ROOT, "include", "tsu_hip_multispin.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tsu_msc_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_hip.MULTISPIN_SIGNATURES)
    lib = _hip.load_library()
    for name in NEW_SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_hip.MULTISPIN_SIGNATURES[name][1]), name
        assert getattr(lib, name).argtypes == _hip.MULTISPIN_SIGNATURES[name][1]
    assert not set(_hip.MULTISPIN_SIGNATURES) & set(_hip.SIGNATURES) and lib.tsu_version() == 100
    with open(os.path.join(ROOT, "tsu-emulator_amd", "csrc", "build.sh")) as f:
        build = f.read()
    for name in ("tsu_hip_multispin.h", "multispin_dev.h"):
        assert name in build, name
    import tsu
    from tsu import models
    for mod in (tsu, models):
        for n in ("MultispinGlass3D", "multispin_scan_3d"):
            assert n in mod.__all__ and getattr(mod, n) is getattr(models.ising, n)


def test_philox_tags_are_unchanged_and_the_kernels_hold_no_exp():
    csrc = os.path.join(ROOT, "tsu-emulator_amd", "csrc")
    with open(os.path.join(csrc, "tsu_common.h")) as f:
        common = f.read()
    assert sorted(int(v) for v in re.findall(r"TSU_TAG_[A-Z_]+\s*=\s*(\d+)", common)) == list(range(13))
    with open(os.path.join(csrc, "multispin_dev.h")) as f:
        dev = re.sub(r"//[^\n]*", "", f.read())
    assert not re.search(r"\bexpf?\s*\(|double|float", dev)
    with open(os.path.join(csrc, "multispin.hip")) as f:
        hip = re.sub(r"//[^\n]*", "", f.read())
    assert len(re.findall(r"\bexp\s*\(", hip)) == 1  # the host table
    assert set(re.findall(r"__global__[^;{]*?\b(k9_\w+)\s*\(", hip)) == {"k9_sweep", "k9_small", "k9_randomize", "k9_measure"}

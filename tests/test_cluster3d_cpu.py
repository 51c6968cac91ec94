"""K8 Swendsen-Wang in 3-D on the host: the NumPy twin (tests/helpers/cluster3d_twin.py) against the 2-D twin on one layer, its
bonds, labels and coins, the Python layer's refusals before the device is touched, and the new symbols (no GPU needed)."""
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


twin = _load("cluster3d_twin")
twin2 = _load("cluster_twin")
lat3 = _load("lattice3d_twin")


def _disorder(kind, shape, periodic, dseed):
    """(J_right, J_down, J_layer) float32; the last slice of an open axis 0."""
    rng = np.random.default_rng(dseed)
    if kind == "ferro":
        j = [np.full(shape, 1.0, np.float32) for _ in range(3)]
    elif kind == "antiferro":
        j = [np.full(shape, -1.0, np.float32) for _ in range(3)]
    elif kind == "gauss":
        j = [rng.normal(size=shape).astype(np.float32) for _ in range(3)]
    elif kind == "pmJ":
        j = [rng.choice(np.array([-1.0, 1.0], np.float32), size=shape) for _ in range(3)]
    elif kind == "diluted":
        j = [np.where(rng.random(shape) < 0.3, 0.0, 1.0).astype(np.float32) for _ in range(3)]
    else:
        raise ValueError(kind)
    pz, pr, pc = twin.axes(periodic)
    if not pc:
        j[0][:, :, -1] = 0.0
    if not pr:
        j[1][:, -1, :] = 0.0
    if not pz:
        j[2][-1, :, :] = 0.0
    return tuple(j)


@pytest.mark.parametrize("rows,cols,periodic", [(8, 12, True), (5, 7, False), (1, 9, False), (6, 4, True)])
@pytest.mark.parametrize("J,T", [(1.0, 2.269), (-1.0, 1.5), (0.5, 4.5)])
def test_one_layer_equals_the_2d_twin(rows, cols, periodic, J, T):
    rng = np.random.default_rng(rows * 100 + cols)
    s = rng.choice(np.array([-1, 1], np.int8), size=(rows, cols))
    per3 = (False, periodic, periodic)
    jr, jd, jl = (np.full((1, rows, cols), J, np.float32) for _ in range(3))
    jl[:] = 0.0
    if not periodic:
        jr[:, :, -1] = 0.0
        jd[:, -1, :] = 0.0
    for replica in (0, 3):
        got = twin.sweep(s[None], per3, jr, jd, jl, T, 5, seed=(7 << 32) | 99, step0=11, replica=replica)
        want = twin2.sweep(s, periodic, J, T, 5, seed=(7 << 32) | 99, step0=11, replica=replica)
        assert (got[0] == want).all()


@pytest.mark.parametrize("kind", ["ferro", "antiferro", "gauss", "pmJ", "diluted"])
@pytest.mark.parametrize("shape,periodic", [((4, 6, 8), True), ((3, 5, 7), False), ((4, 3, 6), (True, False, True))])
def test_active_bonds_join_sites_of_one_label(kind, shape, periodic):
    rng = np.random.default_rng(5)
    s = rng.choice(np.array([-1, 1], np.int8), size=shape)
    j = _disorder(kind, shape, periodic, 9)
    roots, act = twin.labels(s, periodic, *j, 2.0, seed=21, t=4)
    idx = np.arange(s.size).reshape(shape)
    assert (roots <= idx).all() and (roots.ravel()[roots.ravel()] == roots.ravel()).all()
    n_active = 0
    for axis, a, J in zip((2, 1, 0), act, j):
        other = np.roll(roots, -1, axis=axis)
        assert (roots[a] == other[a]).all()
        # an active bond is satisfied and has a nonzero coupling; an open axis has none from its last slice
        assert (J[a] * s[a] * np.roll(s, -1, axis=axis)[a] > 0).all()
        if not twin.axes(periodic)[axis]:
            assert not np.take(a, -1, axis=axis).any()
        n_active += int(a.sum())
    assert n_active > 0
    # the clusters are exactly the components: as many roots as sites minus the bonds of a spanning forest
    for r in np.unique(roots):
        assert idx[roots == r].min() == r


def test_zero_couplings_make_every_site_its_own_cluster():
    shape = (3, 4, 6)
    rng = np.random.default_rng(2)
    s = rng.choice(np.array([-1, 1], np.int8), size=shape)
    z = tuple(np.zeros(shape, np.float32) for _ in range(3))
    for periodic in (False, (False, True, True)):
        roots, act = twin.labels(s, periodic, *z, 1.0, seed=8, t=2)
        assert (roots == np.arange(s.size).reshape(shape)).all() and not any(a.any() for a in act)
        got = twin.step(s, periodic, *z, 1.0, seed=8, t=2)
        coin = twin.flip_of_roots(np.arange(s.size), shape[2], 8, 2).reshape(shape)
        assert (got == np.where(coin, -s, s)).all()
        assert 0 < coin.sum() < s.size


@pytest.mark.parametrize("kind", ["ferro", "antiferro", "pmJ", "gauss"])
def test_cold_step_keeps_the_energy_of_a_satisfied_configuration(kind):
    """T -> 0+ on a configuration that satisfies every bond: every bond with J != 0 is active, whole components flip, E stays."""
    shape = (4, 4, 6)
    periodic = (True, False, True)
    rng = np.random.default_rng(4)
    if kind == "ferro":
        s = np.ones(shape, np.int8)
        j = _disorder("ferro", shape, periodic, 0)
    elif kind == "antiferro":
        s = np.where(lat3.colours(shape) == 0, 1, -1).astype(np.int8)
        j = _disorder("antiferro", shape, periodic, 0)
    else:  # a Mattis model: J_ij = |J_ij| xi_i xi_j is satisfied by s = xi
        s = rng.choice(np.array([-1, 1], np.int8), size=shape)
        mag = _disorder("ferro" if kind == "pmJ" else "gauss", shape, periodic, 6)
        j = tuple((np.abs(m) * s * np.roll(s, -1, axis=axis)).astype(np.float32) for axis, m in zip((2, 1, 0), mag))
    e0 = lat3.energy(s, periodic, *j)
    cur = s
    for t in range(4):
        cur = twin.step(cur, periodic, *j, 1e-6, seed=3, t=t)
        assert lat3.energy(cur, periodic, *j) == e0
    assert len(np.unique(twin.labels(s, periodic, *j, 1e-6, seed=3, t=0)[0])) == 1


def test_thresholds():
    j = np.array([0.0, 1.0, -1.0, 0.3, 1e-30, 50.0], np.float32)
    thr = twin.thresholds(j, 2.0)
    assert thr[0] == 0 and thr[1] == thr[2] == twin2.threshold(1.0, 2.0)
    assert thr[3] == twin2.threshold(float(np.float32(0.3)), 2.0)
    assert thr[5] == 2 ** 32  # p rounds to 1: the compare is 64-bit
    assert twin.thresholds(np.float32(1.0), 1e-300) == 2 ** 32
    with pytest.raises(ValueError, match="Temperature must be positive"):
        twin.thresholds(j, 0.0)


def test_cluster_validation_before_the_device():
    from tsu import _hip
    from tsu.models import ising

    def fake(field=None):
        m = ising.IsingModel3D.__new__(ising.IsingModel3D)
        m.shape = (2, 2, 4)
        m.temperature, m.seed, m.cluster_count, m.sweep_count = 2.0, 1, 0, 0
        m._disorder = (None, None, None, field)
        m._lat = None  # any device access would raise AttributeError
        return m

    h = np.zeros((2, 2, 4), np.float32)
    h[1, 0, 2] = 0.25
    with pytest.raises(_hip.UnsupportedError, match="ghost spin"):
        fake(h).cluster_update(1)
    with pytest.raises(_hip.UnsupportedError, match="ghost spin"):
        fake(h).equilibrate(n_sweeps=3, algorithm="swendsen_wang")
    with pytest.raises(ValueError, match="algorithm"):
        fake().equilibrate(n_sweeps=3, algorithm="wolff")
    for T in (0.0, -1.0):
        with pytest.raises(ValueError, match="Temperature must be positive"):
            fake().equilibrate(T, n_sweeps=3, algorithm="swendsen_wang")
    # an all-zero field array is zero field: the call goes on to the device (here: to the missing handle)
    with pytest.raises(AttributeError):
        fake(np.zeros((2, 2, 4), np.float32)).cluster_update(1)
    with pytest.raises(ValueError, match="algorithm"):
        ising.temperature_scan_3d(4, [2.0], algorithm="metropolis")
    with pytest.raises(_hip.UnsupportedError, match="ghost spin"):
        ising.temperature_scan_3d((2, 2, 4), [2.0], periodic=False, field=h, algorithm="swendsen_wang")
    with pytest.raises(ValueError, match="Temperature must be positive"):
        ising.temperature_scan_3d(4, [2.0, 0.0], algorithm="swendsen_wang")


NEW_SYMBOLS = ("tsu_ising3d_cluster_sweep", "tsu_ising3d_cluster_sweep_batch", "tsu_ising3d_cluster_launch_count")


def test_new_symbols_in_header_library_and_signatures():
    """The cluster entry points are declared in include/tsu_hip_ising3d_cluster.h, which tsu_hip.h includes, exported by the
    library, and prototyped one to one in _hip.CLUSTER3D_SIGNATURES (which load_library declares)."""
    from tsu import _hip
    with open(os.path.join(ROOT, "include", "tsu_hip.h")) as f:
        main = f.read()
    assert re.search(r'^#include "tsu_hip_ising3d_cluster.h"', main, flags=re.M)
    with open(os.path.join(ROOT, "include", "tsu_hip_ising3d_cluster.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tsu_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_hip.CLUSTER3D_SIGNATURES)
    lib = _hip.load_library()
    for name in NEW_SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_hip.CLUSTER3D_SIGNATURES[name][1]), name
        fn = getattr(lib, name)
        assert fn.argtypes == _hip.CLUSTER3D_SIGNATURES[name][1]
    assert len(_hip.CLUSTER3D_SIGNATURES["tsu_ising3d_cluster_sweep"][1]) == 6
    assert len(_hip.CLUSTER3D_SIGNATURES["tsu_ising3d_cluster_sweep_batch"][1]) == 7
    for name in ("cluster_sweep", "cluster_launch_count"):
        assert callable(getattr(_hip.Lattice3D, name))
    assert callable(_hip.cluster_sweep_batch_3d)


def test_layer_tag_is_10_in_both_places():
    with open(os.path.join(ROOT, "tsu-emulator_amd", "csrc", "tsu_common.h")) as f:
        common = f.read()
    assert re.search(r"TSU_TAG_SW_LAYER\s*=\s*10\b", common) and twin.TAG_SW_LAYER == 10
    assert twin.TAG_SW_BOND == 6 and twin.TAG_SW_FLIP == 7

"""Ghost-spin Swendsen-Wang steps on the host: the NumPy twin (tests/helpers/cluster_field_twin.py) against the zero-field twin, its
ghost bonds and frozen components, the thresholds, the Philox tag, the new header and ctypes prototypes, and the Python layer's
validation before the device is touched (no GPU needed)."""
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


twin = _load("cluster_field_twin")
twin0 = _load("cluster3d_twin")
lat3 = _load("lattice3d_twin")

KINDS = ["ferro", "antiferro", "gauss", "pmJ", "diluted"]


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
    pz, pr, pc = twin0.axes(periodic)
    if not pc:
        j[0][:, :, -1] = 0.0
    if not pr:
        j[1][:, -1, :] = 0.0
    if not pz:
        j[2][-1, :, :] = 0.0
    return tuple(j)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,periodic", [((3, 5, 7), False), ((4, 4, 8), True)])
def test_zero_field_is_the_zero_field_twin(kind, shape, periodic):
    rng = np.random.default_rng(3)
    s = rng.choice(np.array([-1, 1], np.int8), size=shape)
    j = _disorder(kind, shape, periodic, 9)
    for h in (None, np.zeros(shape, np.float32)):
        for replica in (0, 3):
            for t in (0, 17):
                got = twin.step(s, periodic, *j, h, 2.0, seed=(5 << 32) | 21, t=t, replica=replica)
                want = twin0.step(s, periodic, *j, 2.0, seed=(5 << 32) | 21, t=t, replica=replica)
                assert (got == want).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,periodic", [((3, 5, 7), False), ((4, 4, 8), True), ((1, 6, 10), (False, True, True))])
def test_frozen_components_stay_and_free_ones_flip_whole(kind, shape, periodic):
    rng = np.random.default_rng(4)
    s = rng.choice(np.array([-1, 1], np.int8), size=shape)
    j = _disorder(kind, shape, periodic, 9)
    h = rng.normal(size=shape).astype(np.float32)
    h[rng.random(shape) < 0.3] = 0.0
    T, seed = 1.5, 77
    seen_frozen = seen_flip = 0
    for t in range(6):
        roots, frozen, act, ghost = twin.labels(s, periodic, *j, h, T, seed, t)
        new = twin.step(s, periodic, *j, h, T, seed, t)
        # an active ghost bond is satisfied and has a nonzero field; its site is frozen and never changes
        assert (h[ghost] * s[ghost] > 0).all() and frozen[ghost].all()
        assert (new[ghost] == s[ghost]).all() and (new[frozen] == s[frozen]).all()
        # the lattice bonds are those of the zero-field step; both ends of one share root and frozen flag
        act0 = twin0.active_bonds(s, periodic, *j, T, seed, t)
        for axis, a, a0 in zip((2, 1, 0), act, act0):
            assert (a == a0).all()
            assert (roots[a] == np.roll(roots, -1, axis=axis)[a]).all() and (frozen[a] == np.roll(frozen, -1, axis=axis)[a]).all()
        # every frozen component holds an active ghost bond; every flipped site lies in a component without one
        for r in np.unique(roots[frozen]):
            assert ghost[roots == r].any()
        flipped = new != s
        assert not frozen[flipped].any()
        for r in np.unique(roots[~frozen]):
            assert not ghost[roots == r].any()
            coin = bool(twin.flip_of_roots(np.array([r]), shape[2], seed, t)[0])
            assert (flipped[roots == r] == coin).all()
        seen_frozen += int(frozen.sum())
        seen_flip += int(flipped.sum())
        s = new
    assert seen_frozen > 0 and seen_flip > 0


def test_ghost_bond_needs_a_field_along_the_spin():
    shape = (2, 3, 4)
    s = np.ones(shape, np.int8)
    s[1] = -1
    h = np.full(shape, 50.0, np.float32)  # thr = 2^32: every satisfied ghost bond is active
    g = twin.active_ghost(s, h, 1.0, 3, 0)
    assert g[0].all() and not g[1].any()
    assert (twin.active_ghost(s, -h, 1.0, 3, 0) == ~g).all()
    assert not twin.active_ghost(s, np.zeros(shape, np.float32), 1.0, 3, 0).any()
    assert not twin.active_ghost(s, None, 1.0, 3, 0).any()


def test_ghost_thresholds_reach_two_to_the_32():
    h = np.array([0.0, 0.05, -0.05, 1e-30, 40.0, -40.0], np.float32)
    thr = twin.thresholds(np.abs(h), 2.0)
    assert thr.dtype == np.uint64 and thr[0] == 0 and thr[1] == thr[2] and 0 < thr[1] < 2 ** 32
    assert thr[4] == thr[5] == 2 ** 32  # p rounds to 1: u_g < thr is a 64-bit compare, true for every u_g
    assert twin.thresholds(np.float32(0.01), 1e-300) == 2 ** 32
    assert thr[1] == int(np.floor(-np.expm1(-2.0 * float(np.float32(0.05)) / 2.0) * 4294967296.0))
    u = twin.ghost_uniforms((2, 3, 9), 5, 1)
    assert u.dtype == np.uint64 and (u < 2 ** 32).all() and len(np.unique(u)) == u.size


def test_ghost_uniforms_are_their_own_stream():
    """word c & 3 of Philox(c >> 2, rho, t, 12 | replica << 8): the layer bonds' layout under another tag."""
    shape, seed, t = (3, 4, 10), (9 << 32) | 4, 6
    u = twin.ghost_uniforms(shape, seed, t, replica=2)
    for (z, r, c) in ((0, 0, 0), (1, 3, 5), (2, 2, 9)):
        w = twin.philox4x32_10(c >> 2, z * 4 + r, t, 12 | (2 << 8), seed & 0xFFFFFFFF, seed >> 32)
        assert int(u[z, r, c]) == int(w[c & 3])
    assert (u != twin0.bond_uniforms(shape, seed, t, 2)[2]).any()
    assert (u != twin.ghost_uniforms(shape, seed, t, replica=0)).any()


def test_ghost_tag_is_12_in_both_places():
    with open(os.path.join(ROOT, "tsu-emulator_amd", "csrc", "tsu_common.h")) as f:
        common = f.read()
    assert re.search(r"TSU_TAG_SW_GHOST\s*=\s*12\b", common) and twin.TAG_SW_GHOST == 12
    tags = [int(v) for v in re.findall(r"TSU_TAG_[A-Z_]+\s*=\s*(\d+)", common)]
    assert sorted(tags) == list(range(13))  # 12 is new, nothing else moved


NEW_SYMBOLS = ("tsu_ising3d_cluster_sweep_field", "tsu_ising3d_cluster_sweep_field_batch")
OLD_CLUSTER3D = ("tsu_ising3d_cluster_sweep", "tsu_ising3d_cluster_sweep_batch", "tsu_ising3d_cluster_launch_count")


def test_header_and_ctypes_prototypes_agree():
    """The entry points are declared in include/tsu_hip_cluster_field.h, which tsu_hip.h includes after tsu_hip_probe.h and build.sh
    lists, exported by the library and prototyped one to one in _hip.CLUSTER_FIELD_SIGNATURES (which load_library declares); the
    zero-field header and CLUSTER3D_SIGNATURES keep their three."""
    from tsu import _hip
    with open(os.path.join(ROOT, "include", "tsu_hip.h")) as f:
        top = f.read()
    assert re.search(r'^#include "tsu_hip_cluster_field.h"', top, flags=re.M)
    assert top.index('#include "tsu_hip_probe.h"') < top.index('#include "tsu_hip_cluster_field.h"')
    with open(os.path.join(ROOT, "include", "tsu_hip_cluster_field.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tsu_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_hip.CLUSTER_FIELD_SIGNATURES)
    lib = _hip.load_library()
    for name in NEW_SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_hip.CLUSTER_FIELD_SIGNATURES[name][1]), name
        assert getattr(lib, name).argtypes == _hip.CLUSTER_FIELD_SIGNATURES[name][1]
    assert len(_hip.CLUSTER_FIELD_SIGNATURES["tsu_ising3d_cluster_sweep_field"][1]) == 6
    assert len(_hip.CLUSTER_FIELD_SIGNATURES["tsu_ising3d_cluster_sweep_field_batch"][1]) == 7
    assert sorted(_hip.CLUSTER3D_SIGNATURES) == sorted(OLD_CLUSTER3D)
    with open(os.path.join(ROOT, "include", "tsu_hip_ising3d_cluster.h")) as f:
        old = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(tsu_[a-z0-9_]+)\s*\(", old))) == sorted(OLD_CLUSTER3D)
    with open(os.path.join(ROOT, "tsu-emulator_amd", "csrc", "build.sh")) as f:
        assert "tsu_hip_cluster_field.h" in f.read()
    assert callable(_hip.Lattice3D.cluster_sweep_field) and callable(_hip.cluster_sweep_field_batch_3d)


def test_ghost_validation_before_the_device():
    from tsu import _hip
    from tsu.models import ising

    def fake3(field=None):
        m = ising.IsingModel3D.__new__(ising.IsingModel3D)
        m.shape = (2, 2, 4)
        m.temperature, m.seed, m.cluster_count, m.sweep_count = 2.0, 1, 0, 0
        m._disorder = (None, None, None, field)
        m._lat = None  # any device access would raise AttributeError
        return m

    def fake2():
        m = ising.IsingModel2D.__new__(ising.IsingModel2D)
        m.rows, m.cols, m.coupling, m.external_field, m.bias_mode = 4, 6, 1.0, 0.1, "physical"
        m.temperature, m.seed, m.cluster_count, m.sweep_count = 2.0, 1, 0, 0
        m._disorder = None
        m._lat = None
        return m

    h = np.zeros((2, 2, 4), np.float32)
    h[1, 0, 2] = 0.25
    with pytest.raises(ValueError, match="algorithm"):
        fake3(h).equilibrate(n_sweeps=3, algorithm="wolff")
    with pytest.raises(ValueError, match="algorithm"):
        ising.temperature_scan_3d(4, [2.0], algorithm="swendsen_wang_ghosts")
    for T in (0.0, -1.0):
        with pytest.raises(ValueError, match="Temperature must be positive"):
            fake3(h).equilibrate(T, n_sweeps=3, algorithm="swendsen_wang_ghost")
        with pytest.raises(ValueError, match="Temperature must be positive"):
            ising.temperature_scan_3d((2, 2, 4), [2.0, T], periodic=False, field=h, algorithm="swendsen_wang_ghost")
    # a field passes the host checks of the ghost algorithm: the call goes on to the device (here: to the missing handle)
    with pytest.raises(AttributeError):
        fake3(h).equilibrate(n_sweeps=3, algorithm="swendsen_wang_ghost")
    with pytest.raises(AttributeError):
        fake3(h).ghost_cluster_update(1)
    # the zero-field algorithm still refuses it
    with pytest.raises(_hip.UnsupportedError, match="ghost spin"):
        fake3(h).equilibrate(n_sweeps=3, algorithm="swendsen_wang")
    # the 2-D facade names the one-layer route
    hint = re.escape("IsingModel3D(size=(1, R, C), periodic=(False, p, p))")
    with pytest.raises(_hip.UnsupportedError, match=hint):
        fake2().equilibrate(n_sweeps=3, algorithm="swendsen_wang_ghost")
    with pytest.raises(_hip.UnsupportedError, match=hint):
        ising.temperature_scan(8, [2.0], algorithm="swendsen_wang_ghost")
    with pytest.raises(ValueError, match="algorithm"):
        fake2().equilibrate(n_sweeps=3, algorithm="wolff")

"""K9 tempering on the host: the twin's masked exchange against a per-sample permutation, its swap pass against K7's, its integers
against the per-sample energies, the Python layer's refusals before the device is touched, and the new header and ctypes
prototypes (no GPU needed)."""
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


twin = _load("multispin_pt_twin")
msc = twin.msc


@pytest.mark.parametrize("R,A,S", [(2, 1, 1), (5, 2, 70), (9, 1, 130)])
def test_masked_exchange_is_a_permutation_per_sample(R, A, S):
    """Random masks, then a pass in which every pair accepts (the slot-0 configuration arrives at the top, every other one moves
    down by one), none does, and runs of consecutive accepts that differ from bit to bit."""
    rng = np.random.default_rng(R * 1000 + S)
    shape = (2, 3, 5)
    bits = rng.integers(0, 2, size=(R, A, S) + shape).astype(bool)
    planes = np.stack([np.stack([msc.pack(bits[t, a]) for a in range(A)]) for t in range(R)])
    W = (S + 63) // 64
    pad = planes.copy()
    if S % 64:  # pad bits that are set must stay where they are
        pad[:, :, -1] |= rng.integers(0, 2 ** 63, size=pad[:, :, -1].shape, dtype=np.uint64) << np.uint64(S % 64)
    cases = [rng.integers(0, 2, size=(R - 1, A, S)).astype(bool) for _ in range(4)]
    cases += [np.ones((R - 1, A, S), bool), np.zeros((R - 1, A, S), bool)]
    runs = np.zeros((R - 1, A, S), bool)
    for s in range(S):
        runs[:1 + s % R, :, s] = True  # sample s: the first 1 + s % R pairs accept, so its slot-0 configuration climbs that far
    cases.append(runs[:R - 1])
    for accept in cases:
        masks = twin.pack_masks(accept)
        assert masks.shape == (R - 1, A, W) and masks.dtype == np.uint64
        if S % 64:
            assert not np.any(masks[:, :, -1] >> np.uint64(S % 64))
        got = twin.exchange(planes, masks)
        want = twin.exchange_unpacked(bits, accept)
        for t in range(R):
            for a in range(A):
                assert (msc.unpack(got[t, a], S) == want[t, a]).all()
        if S % 64:
            moved = twin.exchange(pad, masks)
            keep = ~np.uint64((1 << (S % 64)) - 1)
            assert ((moved[:, :, -1] & keep) == (pad[:, :, -1] & keep)).all()
    top = twin.exchange_unpacked(bits, cases[4])
    assert (top[R - 1] == bits[0]).all() and (top[:R - 1] == bits[1:]).all()


def test_swap_pass_is_k7s_per_sample():
    """Per (replica, sample) the pass is tempering_twin.swap_pass on that sample's energies with its own key: labels are the
    walkers, and the energy of a slot is that of the walker there."""
    R, A, S = 6, 2, 5
    T = np.linspace(0.4, 2.0, R)
    rng = np.random.default_rng(3)
    seeds = [int(x) for x in rng.integers(0, 2 ** 63, size=S)]
    book = twin.Book(A, S, R)
    was = np.tile(np.arange(R), (A, S, 1))
    flags = np.full((A, S, R), twin.NONE)
    flags[:, :, 0] = twin.BOTTOM
    trips = np.zeros((A, S, R), np.int64)
    att, acc = np.zeros((A, S, R - 1), np.int64), np.zeros((A, S, R - 1), np.int64)
    for rnd in range(40):
        E_walker = rng.integers(-3, 4, size=(A, S, R)).astype(np.float64)  # new energies every round: the walkers keep moving
        E_slot = np.zeros((R, A, S))
        for a in range(A):
            for s in range(S):
                E_slot[:, a, s] = E_walker[a, s, book.labels[a, s]]
        before = book.labels.copy()
        accept = twin.swap_pass(book, T, E_slot, seeds)
        for a in range(A):
            for s in range(S):
                u = twin.pt.swap_uniforms(R, rnd, seeds[s], a)
                twin.pt.swap_pass(was[a, s], T, E_walker[a, s], u, att[a, s], acc[a, s], flags[a, s], trips[a, s])
                # the masks reproduce the new order from the old one
                assert (twin.exchange_unpacked(before[a, s][:, None, None], accept[:, a:a + 1, s:s + 1])[:, 0, 0] == book.labels[a, s]).all()
        assert (book.labels == was).all() and (book.flags == flags).all() and (book.trips == trips).all()
        assert (book.attempts == att).all() and (book.accepts == acc).all()
    assert book.rounds == 40 and trips.sum() > 0 and 0 < acc.sum() < att.sum()


def test_twin_integers_are_the_per_sample_ones():
    from tsu.models import edwards_anderson_samples
    for shape, periodic in (((3, 5, 6), False), ((4, 4, 6), (True, False, True))):
        S, R, A = 66, 2, 2
        j = edwards_anderson_samples(shape, S, kind="bimodal", seed=4, periodic=periodic)
        spins = np.random.default_rng(5).choice(np.array([-1, 1], np.int8), size=(R, A, S) + shape)
        planes = np.stack([np.stack([msc.pack(spins[t, a] == 1) for a in range(A)]) for t in range(R)])
        unsat, ssum, q, ql, nb = twin.measure(planes, periodic, *[msc.pack(a == -1) for a in j], S)
        for t in range(R):
            for a in range(A):
                assert (2 * unsat[t, a] - nb == msc.reference_energy(spins[t, a], periodic, j)).all()
                assert (ssum[t, a] == spins[t, a].reshape(S, -1).sum(axis=1)).all()
            p = spins[t, 0].astype(np.int64) * spins[t, 1]
            assert (q[t] == p.reshape(S, -1).sum(axis=1)).all()
            # q_link of a pair is the energy of the product field under J = -1... stated directly: -E(p) with all J = +1
            ones = [np.where(a != 0, 1.0, 0.0) for a in j]
            assert (ql[t] == -msc.reference_energy(p.astype(np.int8), periodic, ones)).all()


def test_cpu_tempering_without_swaps_is_the_sweep():
    from tsu.models import edwards_anderson_samples
    shape, S, T = (4, 4, 4), 3, [0.7, 1.9]
    j = [msc.pack(a == -1) for a in edwards_anderson_samples(shape, S, kind="bimodal", seed=2)]
    start = np.random.default_rng(1).integers(0, 2 ** 63, size=(2, 1, 1) + shape, dtype=np.uint64)
    a = twin.Tempering(start, True, *j, T, [[11], [12]], [5, 6, 7], S)
    a.run(2, 3, swap=False)
    for t in range(2):
        assert (a.planes[t, 0] == msc.bitsliced_sweep(start[t, 0], True, *j, T[t], 6, 11 + t)).all()
    assert a.book.attempts.sum() == 0
    b = twin.Tempering(start, True, *j, T, [[11], [12]], [5, 6, 7], S)
    rows = b.run(4, 1)
    assert rows[0].shape == (4, 2, 1, S) and rows[2] is None and (b.book.attempts == 4).all()


def test_refusals_come_before_the_device(monkeypatch):
    from tsu import _hip
    from tsu.models import MultispinTempering3D, edwards_anderson_samples, multispin_tempering_scan_3d

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_hip, "MultispinLattice", no_device)
    shape = (4, 4, 6)
    j = edwards_anderson_samples(shape, 3, kind="bimodal", seed=1)
    with pytest.raises(ValueError, match="2 to 256 temperatures, got 1"):
        MultispinTempering3D(shape, [1.0], couplings=j)
    with pytest.raises(ValueError, match="2 to 256 temperatures, got 257"):
        MultispinTempering3D(shape, np.linspace(0.5, 3.0, 257), couplings=j)
    with pytest.raises(ValueError, match="not both"):
        MultispinTempering3D(shape, [1.0, 2.0], couplings=j, swap_seed=1, swap_seeds=[1, 2, 3])
    with pytest.raises(ValueError, match=r"one swap seed per sample \(3\), got 2"):
        MultispinTempering3D(shape, [1.0, 2.0], couplings=j, swap_seeds=[1, 2])
    with pytest.raises(ValueError, match="unsigned 64-bit"):
        MultispinTempering3D(shape, [1.0, 2.0], couplings=j, swap_seeds=[1, 2, 2 ** 64])
    with pytest.raises(ValueError, match="unsigned 64-bit"):
        MultispinTempering3D(shape, [1.0, 2.0], couplings=j, swap_seed=2 ** 64 - 2)
    # the glass's own refusals still come first
    with pytest.raises(ValueError, match="J_right.*Gaussian"):
        MultispinTempering3D(shape, [1.0, 2.0], couplings=edwards_anderson_samples(shape, 3, kind="gaussian", seed=1))
    with pytest.raises(ValueError, match="Temperature must be positive"):
        MultispinTempering3D(shape, [1.0, 0.0], couplings=j)
    with pytest.raises(ValueError, match="replicas"):
        MultispinTempering3D(shape, [1.0, 2.0], couplings=j, replicas=3)
    for kw in (dict(swap_interval=0), dict(swap_interval=3), dict(swap_interval=4, n_equilibrate=10)):
        with pytest.raises(ValueError, match="swap_interval"):
            multispin_tempering_scan_3d(shape, [1.0, 2.0], couplings=j, measure_every=4, **{"n_equilibrate": 8, **kw})
    with pytest.raises(ValueError, match="replicas"):
        multispin_tempering_scan_3d(shape, [1.0, 2.0], couplings=j, replicas=0)
    # valid input reaches the handle
    with pytest.raises(AssertionError, match="the device was touched"):
        MultispinTempering3D(shape, [1.0, 2.0], couplings=j, replicas=2, seed=1)
    with pytest.raises(AssertionError, match="the device was touched"):
        MultispinTempering3D(shape, [1.0, 2.0], couplings=j, seed=2 ** 64 - 1, swap_seeds=[0, 2 ** 64 - 1, 5])


def test_default_swap_seeds(monkeypatch):
    """swap_seeds[s] = swap_seed + s, and swap_seed = seed + 2 n_temps unless given: the first value past the sweep seeds."""
    from tsu import _hip
    from tsu.models import MultispinTempering3D, edwards_anderson_samples
    seen = {}

    class Stop(Exception):
        pass

    def handle(*a, **k):
        raise Stop()

    monkeypatch.setattr(_hip, "MultispinLattice", handle)
    orig = MultispinTempering3D._before_device

    def spy(self):
        orig(self)
        seen["swap"], seen["sweep"] = list(self.swap_seeds), self.seeds

    monkeypatch.setattr(MultispinTempering3D, "_before_device", spy)
    shape = (4, 4, 6)
    j = edwards_anderson_samples(shape, 3, kind="bimodal", seed=1)
    for kw, want in ((dict(seed=100), [106, 107, 108]), (dict(seed=100, swap_seed=7), [7, 8, 9]),
                     (dict(seeds=[[50, 60], [51, 61], [52, 62]]), [56, 57, 58]), (dict(seed=1, swap_seeds=[9, 9, 2 ** 64 - 1]), [9, 9, 2 ** 64 - 1])):
        with pytest.raises(Stop):
            MultispinTempering3D(shape, [1.0, 2.0, 3.0], couplings=j, replicas=2, **kw)
        assert seen["swap"] == want
    assert max(int(x) for x in seen["sweep"].ravel()) < 106


NEW_SYMBOLS = ("tsu_msc_pt_enable", "tsu_msc_pt_set_swap_seeds", "tsu_msc_pt_run", "tsu_msc_pt_stats", "tsu_msc_pt_history",
               "tsu_msc_pt_launch_count")


def test_header_and_ctypes_prototypes_agree():
    """The entry points are declared in include/tsu_hip_multispin_pt.h, which tsu_hip.h includes after tsu_hip_multispin.h and build.sh
    lists with the internal header, exported by the library and prototyped one to one in _hip.MULTISPIN_PT_SIGNATURES (which
    load_library declares); the older header and dict hold none of them."""
    from tsu import _hip
    with open(os.path.join(ROOT, "include", "tsu_hip.h")) as f:
        top = f.read()
    assert re.search(r'^#include "tsu_hip_multispin_pt.h"', top, flags=re.M)
    assert top.index('#include "tsu_hip_multispin.h"') < top.index('#include "tsu_hip_multispin_pt.h"')
    with open(os.path.join(ROOT, "include", "tsu_hip_multispin_pt.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tsu_msc_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_hip.MULTISPIN_PT_SIGNATURES)
    lib = _hip.load_library()
    for name in NEW_SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_hip.MULTISPIN_PT_SIGNATURES[name][1]), name
        assert getattr(lib, name).argtypes == _hip.MULTISPIN_PT_SIGNATURES[name][1]
    assert not set(_hip.MULTISPIN_PT_SIGNATURES) & (set(_hip.SIGNATURES) | set(_hip.MULTISPIN_SIGNATURES)) and lib.tsu_version() == 100
    with open(os.path.join(ROOT, "tsu-emulator_amd", "csrc", "build.sh")) as f:
        build = f.read()
    for name in ("tsu_hip_multispin_pt.h", "multispin_host.h"):
        assert name in build, name
    import tsu
    from tsu import models
    for mod in (tsu, models):
        for n in ("MultispinTempering3D", "multispin_tempering_scan_3d"):
            assert n in mod.__all__ and getattr(mod, n) is getattr(models.ising, n)
        assert mod.__all__[-2:] == ["MultispinTempering3D", "multispin_tempering_scan_3d"]
    assert issubclass(models.MultispinTempering3D, models.MultispinGlass3D)


def test_philox_tags_are_unchanged_and_the_kernels_are_where_they_belong():
    csrc = os.path.join(ROOT, "tsu-emulator_amd", "csrc")
    with open(os.path.join(csrc, "tsu_common.h")) as f:
        common = f.read()
    assert sorted(int(v) for v in re.findall(r"TSU_TAG_[A-Z_]+\s*=\s*(\d+)", common)) == list(range(13))
    with open(os.path.join(csrc, "multispin_pt.hip")) as f:
        hip = re.sub(r"//[^\n]*", "", f.read())
    assert set(re.findall(r"__global__[^;{]*?\b(k9_\w+)\s*\(", hip)) == {"k9_pt_plan", "k9_pt_apply"}
    assert "TSU_TAG_PT_SWAP" in hip
    with open(os.path.join(csrc, "multispin_host.h")) as f:
        host = re.sub(r"//[^\n]*", "", f.read())
    assert "struct tsu_msc {" in host and "__global__" not in host

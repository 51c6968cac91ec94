"""Tempering ensembles on the GPU (tsu_pte2d_* / tsu_pte3d_*, csrc/pte_host.h): sample s of an ensemble equals the standalone ladder
(LatticeTempering / LatticeTempering3D) on that sample's disorder with seed = seeds[s] bit for bit -- spins at every slot, E, M, q,
walker, q_link, modes, attempts, accepts, round trips, the slot tables and the counters -- for every walker group the sweeps use;
the same with 129 temperatures, and at the ceiling of 65535 walkers; seeds and disorders vary independently; split runs, S = 1
and swap=False; the spins round trip; the launch count; errors; the scan.
The ladders' own tests compare them with the NumPy twins and with exact enumeration, so identity with the ladders carries those
checks over to every sample."""
import importlib.util
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _long_ladder():
    """tests/helpers/long_ladder.py, one instance per process (the long-ladder tests share it)."""
    name = "tsu_tests_long_ladder"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "long_ladder.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


TS = [0.4, 0.9, 1.5, 2.27, 5.0]
SEEDS = [7, 2 ** 32 + 9, 3]  # the high key word, and seeds that are not consecutive
SHAPES_3D = [((4, 4, 4), True), ((3, 5, 37), False), ((8, 6, 40), (True, False, True))]
# the shape list of the 2-D ladders' parity test (tests/test_tempering_gpu.py), by value
SHAPES_2D = [((6, 10), True), ((37, 53), False), ((1, 9), False), ((9, 1), False), ((128, 1000), True), ((1024, 1024), True)]
HIST_KEYS = ("E", "M", "walker", "q", "q_link", "modes")
STAT_KEYS = ("attempts", "accepts", "round_trips", "walker_at_slot")


@pytest.fixture(scope="module")
def hip():
    from tsu import _hip
    return _hip


def _axes(shape, periodic):
    return (bool(periodic),) * len(shape) if isinstance(periodic, bool) else tuple(periodic)


def _disorder(shape, periodic, n_samples, seed):
    """Gaussian couplings and a Gaussian field, different per sample: ((J_right, J_down[, J_layer]), h), each (S, *shape); the
    bonds across an open boundary are 0, as the lattices ask."""
    rng = np.random.default_rng(seed)
    nj = len(shape)
    js = [rng.normal(size=(n_samples,) + shape).astype(np.float32) for _ in range(nj)]
    per = _axes(shape, periodic)
    for j, a in enumerate(js):  # js[j]: the bonds along axis nj - 1 - j
        axis = nj - 1 - j
        if not per[axis]:
            a[(slice(None),) * (axis + 1) + (-1,)] = 0.0
    return tuple(js), rng.normal(size=(n_samples,) + shape).astype(np.float32)


def _classes(shape):
    from tsu.models import ising
    return (ising.LatticeTempering, ising.LatticeTemperingEnsemble) if len(shape) == 2 else (
        ising.LatticeTempering3D, ising.LatticeTemperingEnsemble3D)


def _flags(shape, periodic, ladders):
    return dict(correlation=any(_axes(shape, periodic)), link_overlap=ladders == 2)


def _record(pt, hist_of, spins_of, stats, energies):
    """Everything the contract names, of one sample: per ladder the history rows and the spins at every slot; the statistics."""
    R, nl = len(pt.temperatures), pt.ladders
    return {"hist": [hist_of(k) for k in range(nl)], "spins": [[spins_of(w, k) for w in range(R)] for k in range(nl)],
            "stats": stats, "E": energies[0], "M": energies[1]}


def _ladder_record(shape, periodic, ladders, js, h, seed, runs=((4, 2),), swap=True, Ts=TS, **flags):
    """The standalone ladder on one disorder: ``runs`` = (n_rounds, swap_interval) one after another, the record after the last."""
    Ladder, _ = _classes(shape)
    pt = Ladder(shape, Ts, couplings=js, field=h, periodic=periodic, seed=seed, initial="random", ladders=ladders, **flags)
    try:
        for n, k in runs:
            pt.run(n, k, swap=swap)
        return _record(pt, lambda k: pt.history(k), pt.spins, pt._pt.stats(), pt._pt.energies())
    finally:
        pt._pt.close()


def _ensemble(shape, periodic, ladders, js, h, seeds, Ts=TS, **flags):
    _, Ensemble = _classes(shape)
    return Ensemble(shape, Ts, couplings=js, field=h, periodic=periodic, seeds=seeds, initial="random", ladders=ladders, **flags)


def _sample_record(ens, s):
    st, (E, M) = ens._pt.stats(), ens._pt.energies()
    stats = {k: (v[s] if k in STAT_KEYS else v) for k, v in st.items()}
    return _record(ens, lambda k: ens.history(sample=s, ladder=k), lambda w, k: ens.spins(s, w, k), stats, (E[s], M[s]))


def _assert_same(got, want, what):
    for k, (hg, hw) in enumerate(zip(got["hist"], want["hist"])):
        assert set(hg) == set(hw), (what, set(hg), set(hw))
        for key in hw:
            assert hg[key].dtype == hw[key].dtype and np.array_equal(hg[key], hw[key], equal_nan=True), f"{what}: {key} of ladder {k}"
    for k, (sg, sw) in enumerate(zip(got["spins"], want["spins"])):
        for w, (a, b) in enumerate(zip(sg, sw)):
            assert np.array_equal(a, b), f"{what}: spins at slot {w} of ladder {k}: {int((a != b).sum())} sites differ"
    for key in STAT_KEYS:
        assert np.array_equal(got["stats"][key], want["stats"][key]), f"{what}: {key}"
    for key in ("sweep_count", "round_count"):
        assert got["stats"][key] == want["stats"][key], f"{what}: {key}"
    assert np.array_equal(got["E"], want["E"]) and np.array_equal(got["M"], want["M"]), f"{what}: energies"


_references = {}


def _reference(shape, periodic, ladders):
    """The three standalone ladders of a case, computed once (they do not depend on the walker group)."""
    key = (shape, periodic, ladders)
    if key not in _references:
        js, h = _disorder(shape, periodic, 3, 100 + sum(shape))
        flags = _flags(shape, periodic, ladders)
        _references[key] = (js, h, [_ladder_record(shape, periodic, ladders, tuple(a[s] for a in js), h[s], SEEDS[s], **flags)
                                    for s in range(3)])
    return _references[key]


# ---------------------------------------------------------------- 1. identity with the ladders
@pytest.mark.parametrize("shape,periodic", SHAPES_3D + SHAPES_2D)
@pytest.mark.parametrize("ladders", [1, 2])
@pytest.mark.parametrize("group", ["1", "3", "nlR"])
def test_every_sample_equals_its_ladder(hip, monkeypatch, shape, periodic, ladders, group):
    """Four recorded rounds of two sweeps with swaps, S = 3, R = 5, modes where an axis is periodic and the link overlap with two
    ladders.  TSU_PT_GROUP=3 with nl R = 10 ends a group inside a sample (walkers 9 | 10 belong to different samples)."""
    js, h, want = _reference(shape, periodic, ladders)
    monkeypatch.setenv("TSU_PT_GROUP", str(ladders * len(TS)) if group == "nlR" else group)
    ens = _ensemble(shape, periodic, ladders, js, h, SEEDS, **_flags(shape, periodic, ladders))
    try:
        ens.run(4, 2)
        full = ens.history()
        assert full["E"].shape == (3, 4, len(TS)) and (("q" in full) == (ladders == 2))
        for s in range(3):
            _assert_same(_sample_record(ens, s), want[s], f"sample {s} of {shape} group {group}")
        assert ens.sweep_count == 8
    finally:
        ens.close()


_long_references = {}


def _long_reference(shape, periodic, ladders):
    key = (shape, periodic, ladders)
    if key not in _long_references:
        Ts = _long_ladder().temperatures(129)
        js, h = _disorder(shape, periodic, 2, 200 + sum(shape))
        flags = _flags(shape, periodic, ladders)
        _long_references[key] = (Ts, js, h, [_ladder_record(shape, periodic, ladders, tuple(a[s] for a in js), h[s], SEEDS[s], Ts=Ts, **flags)
                                             for s in range(2)])
    return _long_references[key]


@pytest.mark.parametrize("shape,periodic", [SHAPES_3D[0], SHAPES_2D[0]])
@pytest.mark.parametrize("ladders", [1, 2])
@pytest.mark.parametrize("group", ["1", "7", "nlR"])
def test_every_sample_equals_its_long_ladder(hip, monkeypatch, shape, periodic, ladders, group):
    """The identity above with S = 2 and 129 temperatures: the swap pass of a (sample, ladder) row takes three trips of its 64 lanes
    and finds its tables at k R offsets, the per-slot passes decode (sample, slot) from grid indices up to 2 x 129, and
    TSU_PT_GROUP=7 leaves ragged groups that end inside a sample (129 = 18 x 7 + 3, 258 = 36 x 7 + 6)."""
    Ts, js, h, want = _long_reference(shape, periodic, ladders)
    monkeypatch.setenv("TSU_PT_GROUP", str(ladders * len(Ts)) if group == "nlR" else group)
    ens = _ensemble(shape, periodic, ladders, js, h, SEEDS[:2], Ts=Ts, **_flags(shape, periodic, ladders))
    try:
        ens.run(4, 2)
        full = ens.history()
        assert full["E"].shape == (2, 4, len(Ts)) and (("q" in full) == (ladders == 2))
        for s in range(2):
            _assert_same(_sample_record(ens, s), want[s], f"sample {s} of {shape} group {group}")
            assert (want[s]["stats"]["walker_at_slot"][:, 64:] != np.arange(64, len(Ts))).any(), "no slot past 63 changed hands"
        assert ens.sweep_count == 8
    finally:
        ens.close()


def _ceiling_handles(hip, shape):
    if len(shape) == 2:
        return hip.TemperingEnsemble, hip.TemperingLattice
    return hip.TemperingEnsemble3D, hip.TemperingLattice3D


@pytest.mark.parametrize("shape", [(2, 2), (2, 2, 2)])
@pytest.mark.parametrize("S,R,ladders", [(257, 255, 1), (127, 256, 2)])
def test_the_walker_ceiling(hip, monkeypatch, shape, S, R, ladders):
    """65535 walkers (257 x 255) and 65024 (127 x 2 x 256) on an open lattice of 4 or 8 sites, the raw handles: the energy passes
    launch a grid of y = S nl R rows and the overlap pass y = S R, at or next to the grid-y limit.  One recorded round of two sweeps
    with swaps on dyadic disorder (tests/helpers/long_ladder.py), different per sample: samples 0, S // 2 and S - 1 equal standalone
    ladders on their disorder and seed -- history, tables, energies, spins at slots 0, 64 and R - 1; every sample's energies are
    finite and its sums of spins even integers within +-N."""
    monkeypatch.delenv("TSU_PT_GROUP", raising=False)
    ll = _long_ladder()
    Ensemble, Ladder = _ceiling_handles(hip, shape)
    N = int(np.prod(shape))
    Ts = ll.temperatures(R)
    per_sample = [ll.dyadic_disorder(shape, False, 1000 + s) for s in range(S)]
    dis = tuple(np.stack([d[j] for d in per_sample]) for j in range(len(shape) + 1))
    picked = (0, S // 2, S - 1)
    for a in picked:
        for b in picked:
            assert a == b or any((dis[j][a] != dis[j][b]).any() for j in range(len(dis)))
    seeds = [5000 + 1000 * s for s in range(S)]
    ens = Ensemble(*shape, False, S, R, ladders)
    try:
        ens.set_disorder(*dis)
        ens.set_temperatures(Ts)
        ens.init(seeds, 0)
        ens.run(1, 2, swap=True, record=True)
        hist, st, (E, M) = ens.history(), ens.stats(), ens.energies()
        assert E.shape == M.shape == (S, ladders, R) and np.isfinite(E).all()
        assert (np.abs(M) <= N).all() and (M % 2 == 0).all()
        assert st["sweep_count"] == 2 and st["round_count"] == 1 and (st["attempts"] == 1).all()
        assert (np.sort(st["walker_at_slot"], axis=-1) == np.arange(R)).all()
        for s in picked:
            one = Ladder(*shape, False, R, ladders)
            try:
                one.set_disorder(*per_sample[s])
                one.set_temperatures(Ts)
                one.init(seeds[s], 0)
                one.run(1, 2, swap=True, record=True)
                h1, s1, (E1, M1) = one.history(), one.stats(), one.energies()
                for key in ("E", "M", "walker"):
                    assert np.array_equal(hist[key][:, s], h1[key]), (s, key)
                if ladders == 2:
                    assert np.array_equal(hist["q"][:, s], h1["q"]), s
                for key in STAT_KEYS:
                    assert np.array_equal(st[key][s], s1[key]), (s, key)
                assert np.array_equal(E[s], E1) and np.array_equal(M[s], M1), s
                for k in range(ladders):
                    for slot in (0, 64, R - 1):
                        got = ens.get_spins(s, k, slot)
                        assert np.array_equal(got, one.get_spins(k, slot)), (s, k, slot)
                        assert E[s, k, st["walker_at_slot"][s, k, slot]] == ll.energy(got, False, per_sample[s])
                assert s1["accepts"].sum() > 0
            finally:
                one.close()
    finally:
        ens.close()


# ---------------------------------------------------------------- 2. what varies between samples
@pytest.mark.parametrize("shape,periodic", [((4, 4, 4), True), ((6, 10), True)])
def test_seeds_and_disorders_vary_independently(hip, shape, periodic):
    js, h = _disorder(shape, periodic, 2, 5)
    same_j, same_h = tuple(np.stack([a[0], a[0]]) for a in js), np.stack([h[0], h[0]])
    flags = _flags(shape, periodic, 2)
    for what, (jj, hh, seeds) in {"one disorder, two seeds": (same_j, same_h, [11, 12 + 2 ** 40]),
                                  "one seed, two disorders": (js, h, [11, 11])}.items():
        ens = _ensemble(shape, periodic, 2, jj, hh, seeds, **flags)
        try:
            ens.run(4, 2)
            rec = [_sample_record(ens, s) for s in range(2)]
        finally:
            ens.close()
        assert not np.array_equal(rec[0]["spins"][0][0], rec[1]["spins"][0][0]), what
        assert not np.array_equal(rec[0]["hist"][0]["E"], rec[1]["hist"][0]["E"]), what
        for s in range(2):
            want = _ladder_record(shape, periodic, 2, tuple(a[s] for a in jj), hh[s], seeds[s], **flags)
            _assert_same(rec[s], want, f"{what}: sample {s}")


# ---------------------------------------------------------------- 3. split runs, S = 1, swaps off
@pytest.mark.parametrize("shape,periodic", [((3, 5, 37), False), ((8, 6, 40), (True, False, True)), ((37, 53), False), ((6, 10), True)])
def test_split_runs_equal_one_run(hip, shape, periodic):
    js, h = _disorder(shape, periodic, 3, 8)
    flags = _flags(shape, periodic, 2)
    a = _ensemble(shape, periodic, 2, js, h, SEEDS, **flags)
    b = _ensemble(shape, periodic, 2, js, h, SEEDS, **flags)
    try:
        a.run(2, 3)
        first = a.history()
        a.run(2, 3)
        b.run(4, 3)
        second, whole = a.history(), b.history()
        for key in whole:
            assert np.array_equal(first[key], whole[key][:, :2], equal_nan=True), key
            assert np.array_equal(second[key], whole[key][:, 2:], equal_nan=True), key
        for s in range(3):
            ra, rb = _sample_record(a, s), _sample_record(b, s)
            ra["hist"] = rb["hist"] = []
            _assert_same(ra, rb, f"sample {s} after 2 + 2 rounds and after 4")
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("shape,periodic", [((4, 4, 4), True), ((37, 53), False)])
@pytest.mark.parametrize("ladders", [1, 2])
def test_one_sample_is_the_ladder(hip, shape, periodic, ladders):
    js, h = _disorder(shape, periodic, 1, 21)
    flags = _flags(shape, periodic, ladders)
    ens = _ensemble(shape, periodic, ladders, js, h, [2 ** 33 + 5], **flags)
    try:
        ens.run(4, 2)
        want = _ladder_record(shape, periodic, ladders, tuple(a[0] for a in js), h[0], 2 ** 33 + 5, **flags)
        _assert_same(_sample_record(ens, 0), want, "the one sample")
    finally:
        ens.close()


@pytest.mark.parametrize("shape,periodic", [((4, 6, 8), True), ((3, 5, 9), False), ((16, 16), True), ((9, 12), False)])
@pytest.mark.parametrize("replicas", [1, 2])
def test_without_swaps_equals_temperature_scan(hip, shape, periodic, replicas):
    """swap=False: sample s is temperature_scan(_3d) with the same arguments, seed = seeds[s], exactly (the ladders' own statement)."""
    from tsu.models import ising
    scan, ens_scan = (ising.temperature_scan, ising.tempering_ensemble_scan) if len(shape) == 2 else (
        ising.temperature_scan_3d, ising.tempering_ensemble_scan_3d)
    js, h = _disorder(shape, periodic, 3, 3)
    kw = dict(n_equilibrate=20, n_measure=6, measure_every=4, initial="random", periodic=periodic, replicas=replicas)
    Ts = [0.8, 1.5, 3.0]
    out = ens_scan(shape, Ts, couplings=js, field=h, seeds=SEEDS, swap=False, **kw)
    for s in range(3):
        ref = scan(shape, Ts, couplings=tuple(a[s] for a in js), field=h[s], seed=SEEDS[s], **kw)
        for key in ref:
            if key != "temperatures":
                assert np.array_equal(out[key][s], ref[key], equal_nan=True), (s, key)
    assert np.isnan(out["swap_acceptance"]).all() and not out["round_trips"].any()


# ---------------------------------------------------------------- 4. spins round trip, launch count
@pytest.mark.parametrize("shape,periodic", [((3, 5, 37), False), ((37, 53), False)])
def test_set_spins_reaches_one_plane_only(hip, shape, periodic):
    js, h = _disorder(shape, periodic, 3, 4)
    ens = _ensemble(shape, periodic, 2, js, h, SEEDS)
    try:
        ens.run(2, 1)
        R = len(TS)
        before = {(s, k, w): ens.spins(s, w, k) for s in range(3) for k in range(2) for w in range(R)}
        new = (2 * np.random.default_rng(1).integers(0, 2, size=shape) - 1).astype(np.int8)
        ens._pt.set_spins(2, 1, 3, new)
        for (s, k, w), old in before.items():
            assert np.array_equal(ens.spins(s, w, k), new if (s, k, w) == (2, 1, 3) else old), (s, k, w)
        with pytest.raises(ValueError, match="out of range"):
            ens._pt.get_spins(3, 0, 0)
        with pytest.raises(ValueError, match="out of range"):
            ens._pt.set_spins(0, 2, 0, new)
        with pytest.raises(ValueError, match="out of range"):
            ens.spins(0, R)
    finally:
        ens.close()


@pytest.mark.parametrize("shape,periodic", [((4, 4, 4), True), ((6, 10), True)])
def test_launch_count_does_not_grow_with_samples(hip, shape, periodic):
    counts = []
    for S in (1, 5):
        js, h = _disorder(shape, periodic, S, 6)
        ens = _ensemble(shape, periodic, 2, js, h, list(range(10, 10 + S)))
        try:
            ens.run(3, 4)
            counts.append(ens._pt.launch_count())
        finally:
            ens.close()
    js, h = _disorder(shape, periodic, 1, 6)
    Ladder, _ = _classes(shape)
    pt = Ladder(shape, TS, couplings=tuple(a[0] for a in js), field=h[0], periodic=periodic, seed=10, ladders=2)
    try:
        pt.run(3, 4)
        assert counts == [pt._pt.launch_count()] * 2 == [2 * 3 * 4] * 2
    finally:
        pt._pt.close()


# ---------------------------------------------------------------- 5. errors
def test_errors(hip):
    from tsu.models.ising import LatticeTemperingEnsemble, LatticeTemperingEnsemble3D
    with pytest.raises(ValueError, match="n_samples"):
        hip.TemperingEnsemble3D(4, 4, 4, True, 0, 4, 1)
    with pytest.raises(ValueError, match="n_samples"):
        hip.TemperingEnsemble(4, 4, True, 0, 4, 1)
    # 128 samples x 2 ladders x 256 temperatures = 65536 walkers: refused before anything is allocated
    with pytest.raises(ValueError, match="65536 walkers"):
        hip.TemperingEnsemble3D(2, 2, 2, False, 128, 256, 2)
    with pytest.raises(ValueError, match="65536 walkers"):
        hip.TemperingEnsemble(2, 2, False, 128, 256, 2)
    for bad in ((4, 257, 1), (4, 1, 1), (4, 4, 3)):
        with pytest.raises(ValueError):
            hip.TemperingEnsemble3D(4, 4, 4, True, *bad)
    with pytest.raises(hip.UnsupportedError, match="even length"):
        hip.TemperingEnsemble3D(5, 4, 8, True, 2, 4, 1)
    shape = (4, 4, 8)
    js, h = _disorder(shape, True, 3, 1)
    with pytest.raises(ValueError, match="samples"):
        LatticeTemperingEnsemble3D(shape, TS, couplings=(js[0], js[1], js[2][:2]), field=h)
    with pytest.raises(ValueError, match="samples"):
        LatticeTemperingEnsemble3D(shape, TS, couplings=js, field=h[:2])
    with pytest.raises(ValueError, match="seed"):
        LatticeTemperingEnsemble3D(shape, TS, couplings=js, field=h, seeds=[1, 2])
    with pytest.raises(ValueError, match="at least one"):
        LatticeTemperingEnsemble3D(shape, TS, couplings=tuple(a[:0] for a in js))
    with pytest.raises(ValueError, match="ladders=2"):
        LatticeTemperingEnsemble3D(shape, TS, couplings=js, field=h, link_overlap=True)
    with pytest.raises(ValueError, match="ladders=2"):
        LatticeTemperingEnsemble((4, 8), TS, couplings=tuple(a[:, 0] for a in js[:2]), link_overlap=True)
    pt = hip.TemperingEnsemble3D(*shape, True, 3, 4, 1)
    try:
        with pytest.raises(ValueError, match="set_disorder"):
            pt.run(1, 1)
        with pytest.raises(ValueError, match="shape"):
            pt.set_disorder(*(a[:2] for a in js))
        with pytest.raises(ValueError, match="non-finite"):
            pt.set_disorder(np.full((3,) + shape, np.inf, np.float32), js[1], js[2])
        with pytest.raises(ValueError, match="set_disorder"):  # a refused disorder leaves none
            pt.run(1, 1)
        pt.set_disorder(*js, h)
        with pytest.raises(ValueError, match="set_temperatures"):
            pt.run(1, 1)
        pt.set_temperatures([0.5, 1.0, 2.0, 3.0])
        with pytest.raises(ValueError, match="init"):
            pt.run(1, 1)
        with pytest.raises(ValueError, match="seeds"):
            pt.init([1, 2])
        with pytest.raises(ValueError, match="initial"):
            pt.init([1, 2, 3], 2)
        with pytest.raises(ValueError, match="two ladders"):
            pt.set_link_overlap(True)
        pt.init([1, 2, 3])
        pt.run(2, 1)  # the handle is still usable
        assert pt.history()["E"].shape == (2, 3, 1, 4) and pt.stats()["sweep_count"] == 2
    finally:
        pt.close()


# ---------------------------------------------------------------- 6. the scan
def test_scan_equals_the_ladder_scans_and_its_summary(hip):
    from tsu.models.ising import edwards_anderson_samples, ensemble_summary, tempering_ensemble_scan_3d, tempering_scan_3d
    shape, S, Ts = (4, 4, 4), 4, [0.6, 1.0, 1.6, 2.4]
    js = edwards_anderson_samples(shape, S, kind="gaussian", seed=2)
    seeds = [40, 50, 60 + 2 ** 35, 70]
    kw = dict(n_equilibrate=20, n_measure=8, measure_every=2, initial="random", replicas=2, correlation=True, link_overlap=True)
    out = tempering_ensemble_scan_3d(shape, Ts, couplings=js, seeds=seeds, **kw)
    for s in range(S):
        ref = tempering_scan_3d(shape, Ts, couplings=tuple(a[s] for a in js), seed=seeds[s], **kw)
        for key in ref:
            if key != "temperatures":
                assert np.array_equal(out[key][s], ref[key], equal_nan=True), (s, key)
    want = ensemble_summary({k: v for k, v in out.items() if k not in ("average", "temperatures")}, 64, shape, (True,) * 3)
    assert set(want) == set(out["average"]) and {"binder", "binder_err", "xi_over_L", "xi_over_L_err", "link_overlap"} <= set(want)
    for key in want:
        assert np.array_equal(out["average"][key], want[key], equal_nan=True), key
    assert out["overlap_sq"].shape == (S, len(Ts)) and out["average"]["binder"].shape == (len(Ts),)

"""Cluster-size records of the Swendsen-Wang steps on the GPU (include/tsu_hip_cluster_measure.h; csrc/sw_dev.h, sw_host.h): every row
bit for bit the Python-integer twin's (tests/helpers/cluster_measure_twin.py) and the spins those of an unmeasured run, on the
one-workgroup route up to its LDS limit, on the multi-tile route with clusters across every seam and wrap, and at the limits of the
words (sum_m4 beyond 2^64, all singletons, everything frozen); batches and the switch; the improved estimators against exact
enumeration; their variance against the plain estimator's; the scans' keys."""
import importlib.util
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mtwin = _load("cluster_measure_twin")
lat3 = _load("lattice3d_twin")

TC2, TC3 = 2.269185, 4.5115
SEED = 77
CALLS = [(0, 1), (1, 3)]  # a one-step call, then three consecutive steps in one call


@pytest.fixture(scope="module")
def hip():
    from tsu import _hip
    return _hip


@pytest.fixture(autouse=True)
def _no_tile_switch(monkeypatch):
    monkeypatch.delenv("TSU_SW_TILE", raising=False)
    monkeypatch.delenv("TSU_SW3D_TILE", raising=False)


def _same_spins(got, want, what):
    assert (got == want).all(), f"{what}: spins differ at {np.argwhere(got != want)[:5].tolist()} ({int((got != want).sum())} sites)"


def _same_rows(rec, recs, what):
    """cluster_record()'s dict against the twin's list of rows, every word."""
    assert len(rec["n_clusters"]) == len(recs), f"{what}: {len(rec['n_clusters'])} rows, {len(recs)} steps"
    for k in mtwin.FIELDS:
        got, want = [int(v) for v in rec[k]], [r[k] for r in recs]
        assert got == want, f"{what}: {k} = {got}, twin {want}"


# ---------------------------------------------------------------- 2-D (K6)
def _run_2d(hip, rows, cols, periodic, J, T, start, calls=CALLS, seed=SEED):
    """A measured and an unmeasured lattice through `calls`; after every call: rows == twin, spins == twin == unmeasured.
    Returns (launches measured, launches unmeasured, the last call's record)."""
    a, b = hip.Lattice(rows, cols, periodic), hip.Lattice(rows, cols, periodic)
    try:
        for lat in (a, b):
            lat.randomize(seed + 1) if start == "random" else lat.fill(1)
        a.cluster_measure(True)
        want, rec = a.get_spins(), None
        for step0, n in calls:
            a.cluster_sweep(J, T, n, seed, step0)
            b.cluster_sweep(J, T, n, seed, step0)
            want, recs = mtwin.sweep_2d(want, periodic, J, T, n, seed, step0)
            what = f"{rows}x{cols} periodic={periodic} J={J} T={T} {start} step0={step0}"
            rec = a.cluster_record()
            _same_rows(rec, recs, what)
            _same_spins(a.get_spins(), want, what)
            _same_spins(b.get_spins(), want, what + " (unmeasured)")
        return a.cluster_launch_count(), b.cluster_launch_count(), rec
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("start", ["up", "random"])
@pytest.mark.parametrize("T", [1.5, TC2, 4.0])
@pytest.mark.parametrize("rows,cols,periodic,J", [(7, 9, False, 1.0), (8, 8, True, 1.0), (6, 10, False, -1.0), (128, 128, True, 1.0)])
def test_2d_small_route(hip, rows, cols, periodic, J, T, start):
    """One workgroup, all steps of a call in one launch, measured or not; 128 x 128 is the LDS limit (16384 sites, 144 KB)."""
    on, off, rec = _run_2d(hip, rows, cols, periodic, J, T, start)
    assert on == off == len(CALLS)
    if J > 0:  # a ferromagnet's clusters are aligned: M_C^2 = |C|^2
        assert rec["sum_m2"].tolist() == rec["sum_size2"].tolist()
    assert (rec["n_frozen"] == 0).all() and (rec["m_frozen"] == 0).all()


@pytest.mark.parametrize("start", ["up", "random"])
@pytest.mark.parametrize("T", [1.5, TC2, 4.0])
@pytest.mark.parametrize("rows,cols,periodic,J", [(20, 34, False, 1.0), (24, 24, True, 1.0), (24, 24, True, -1.0)])
def test_2d_tiled_route_small_tiles(hip, monkeypatch, rows, cols, periodic, J, T, start):
    """8 x 8 tiles (partial ones at 20 x 34): clusters cross the seams and the wrap.  Six launches per step measured (local, count,
    merge, fold, row, resolve), three unmeasured."""
    monkeypatch.setenv("TSU_SW_TILE", "8")
    on, off, _ = _run_2d(hip, rows, cols, periodic, J, T, start)
    steps = sum(n for _, n in CALLS)
    assert (on, off) == (6 * steps, 3 * steps)


def test_2d_one_cluster_beyond_two_to_the_64(hip):
    """272 x 256 periodic (69 632 sites: the multi-tile route on its default 64 x 64 tiles), all up at T = 0.05: one cluster, and
    sum_m4 = N^4 > 2^64 needs the high word (its carry out of the low word included: many workgroups add to it)."""
    N = 272 * 256
    on, off, rec = _run_2d(hip, 272, 256, True, 1.0, 0.05, "up", calls=[(0, 3)])
    assert (on, off) == (18, 9)
    assert rec["n_clusters"].tolist() == [1] * 3 and rec["largest"].tolist() == [N] * 3
    assert rec["sum_size2"].tolist() == rec["sum_m2"].tolist() == [N * N] * 3
    assert list(rec["sum_m4"]) == [N ** 4] * 3 and N ** 4 >> 64 > 0


@pytest.mark.parametrize("tile", [None, "8"])
def test_2d_no_bonds_all_singletons(hip, monkeypatch, tile):
    if tile:
        monkeypatch.setenv("TSU_SW_TILE", tile)
    _, _, rec = _run_2d(hip, 12, 18, True, 0.0, 2.0, "random")
    N = 12 * 18
    for k in ("n_clusters", "sum_size2", "sum_m2", "sum_m4"):
        assert [int(v) for v in rec[k]] == [N] * 3, k
    assert rec["largest"].tolist() == [1] * 3


# ---------------------------------------------------------------- 3-D (K8), zero field and ghost
def _couplings(kind, shape, periodic, dseed=5):
    rng = np.random.default_rng(dseed)
    if kind == "uniform":
        j = [np.full(shape, 1.0, np.float32) for _ in range(3)]
    elif kind == "pmJ":
        j = [rng.choice(np.array([-1.0, 1.0], np.float32), size=shape) for _ in range(3)]
    elif kind == "gauss":
        j = [rng.normal(size=shape).astype(np.float32) for _ in range(3)]
    elif kind == "zero":
        j = [np.zeros(shape, np.float32) for _ in range(3)]
    else:
        raise ValueError(kind)
    pz, pr, pc = mtwin.twin3.axes(periodic)
    if not pc:
        j[0][:, :, -1] = 0.0
    if not pr:
        j[1][:, -1, :] = 0.0
    if not pz:
        j[2][-1, :, :] = 0.0
    return tuple(j)


def _field(ghost, shape, dseed=6):
    """None: the zero-field entry point; else the ghost one with a Gaussian field, a uniform h = 0.05 or an all-zero field."""
    if ghost is None:
        return None
    if ghost == "gauss":
        return np.random.default_rng(dseed).normal(size=shape).astype(np.float32)
    return np.full(shape, {"uniform": 0.05, "zero": 0.0, "strong": 10.0}[ghost], np.float32)


def _temps(kind):
    """Ordered, near the transition, high (a glass has no ordered phase to speak of: cold, middling, hot)."""
    return (3.0, TC3, 8.0) if kind == "uniform" else (0.7, 1.1, 3.0)


def _run_3d(hip, shape, periodic, j, h, T, start, calls=CALLS, seed=SEED):
    """_run_2d for the 3-D handle; h is None: tsu_ising3d_cluster_sweep, else tsu_ising3d_cluster_sweep_field."""
    a, b = hip.Lattice3D(*shape, periodic), hip.Lattice3D(*shape, periodic)
    try:
        for lat in (a, b):
            lat.randomize(seed + 1) if start == "random" else lat.fill(1)
            lat.set_disorder(*j) if h is None else lat.set_disorder(*j, h)
        a.cluster_measure(True)
        want, rec = a.get_spins(), None
        for step0, n in calls:
            for lat in (a, b):
                lat.cluster_sweep(T, n, seed, step0) if h is None else lat.cluster_sweep_field(T, n, seed, step0)
            if h is None:
                want, recs = mtwin.sweep_3d(want, periodic, *j, T, n, seed, step0)
            else:
                want, recs = mtwin.sweep_field(want, periodic, *j, h, T, n, seed, step0)
            what = f"{shape} periodic={periodic} T={T} {start} step0={step0}"
            rec = a.cluster_record()
            _same_rows(rec, recs, what)
            _same_spins(a.get_spins(), want, what)
            _same_spins(b.get_spins(), want, what + " (unmeasured)")
        return a.cluster_launch_count(), b.cluster_launch_count(), rec
    finally:
        a.close()
        b.close()


GHOSTS = [None, "gauss", "uniform", "zero"]


@pytest.mark.parametrize("ghost", GHOSTS)
@pytest.mark.parametrize("kind", ["uniform", "pmJ", "gauss"])
@pytest.mark.parametrize("shape,periodic", [((3, 5, 6), False), ((4, 6, 10), (True, False, True))])
def test_3d_small_route(hip, shape, periodic, kind, ghost):
    j, h = _couplings(kind, shape, periodic), _field(ghost, shape)
    frozen = 0
    for T in _temps(kind):
        for start in ("up", "random"):
            on, off, rec = _run_3d(hip, shape, periodic, j, h, T, start)
            assert on == off == len(CALLS)
            frozen += int(rec["n_frozen"].sum())
            if kind == "uniform":
                assert rec["sum_m2"].tolist() == rec["sum_size2"].tolist()
            if ghost in (None, "zero"):
                assert (rec["n_frozen"] == 0).all() and (rec["m_frozen"] == 0).all()
    assert (frozen > 0) == (ghost in ("gauss", "uniform"))  # the ghost cases are not vacuous


@pytest.mark.parametrize("ghost", GHOSTS)
@pytest.mark.parametrize("kind", ["uniform", "pmJ", "gauss"])
def test_3d_small_route_at_the_lds_limit(hip, kind, ghost):
    """16 x 32 x 32 periodic: 16384 sites, 144 KB of LDS with the roots' counts."""
    shape = (16, 32, 32)
    j, h = _couplings(kind, shape, True), _field(ghost, shape)
    Ts = _temps(kind)
    for T, start in ((Ts[0], "up"), (Ts[1], "random"), (Ts[2], "random")):
        on, off, _ = _run_3d(hip, shape, True, j, h, T, start, calls=[(0, 3)])
        assert on == off == 1


@pytest.mark.parametrize("kind,ghost", [("uniform", None), ("pmJ", "gauss"), ("gauss", "uniform"), ("uniform", "zero"), ("uniform", "gauss")])
@pytest.mark.parametrize("shape,periodic", [((8, 8, 12), True), ((5, 9, 14), (False, False, True)), ((6, 9, 14), (True, False, False))])
@pytest.mark.parametrize("tile", ["2x2x2", "3x5x6", "4x4x4"])
def test_3d_tiled_route_small_tiles(hip, monkeypatch, tile, shape, periodic, kind, ghost):
    """Forced small tiles: clusters, frozen ones too, cross the seams of all three axes and the wraps.  Six launches per step
    measured, three unmeasured.  The handle wraps even axes only, so the odd 5 x 9 x 14 wraps along its columns and the wrap in z
    is taken on 6 x 9 x 14."""
    monkeypatch.setenv("TSU_SW3D_TILE", tile)
    j, h = _couplings(kind, shape, periodic), _field(ghost, shape)
    Ts = _temps(kind)
    steps = sum(n for _, n in CALLS)
    for T, start in ((Ts[0], "up"), (Ts[1], "random"), (Ts[2], "random")):
        on, off, _ = _run_3d(hip, shape, periodic, j, h, T, start)
        assert (on, off) == (6 * steps, 3 * steps)


@pytest.mark.parametrize("ghost", [None, "uniform"])
def test_3d_default_tile_above_the_small_limit(hip, ghost):
    """32^3 periodic with no switch set: over the one-workgroup limit, the default tile."""
    shape = (32, 32, 32)
    on, off, _ = _run_3d(hip, shape, True, _couplings("uniform", shape, True), _field(ghost, shape), TC3, "random", calls=[(0, 3)])
    assert (on, off) == (18, 9)


def test_3d_one_tile_has_no_merge_and_no_fold(hip, monkeypatch):
    """A forced tile that holds the whole open lattice: no seam, so no merge pass and no fold: 4 launches per step, 2 unmeasured."""
    monkeypatch.setenv("TSU_SW3D_TILE", "4x6x8")
    shape = (3, 5, 6)
    on, off, _ = _run_3d(hip, shape, False, _couplings("gauss", shape, False), _field("gauss", shape), 1.1, "random")
    steps = sum(n for _, n in CALLS)
    assert (on, off) == (4 * steps, 2 * steps)


@pytest.mark.parametrize("tile", [None, "2x2x2"])
def test_3d_no_bonds_all_singletons(hip, monkeypatch, tile):
    if tile:
        monkeypatch.setenv("TSU_SW3D_TILE", tile)
    shape = (4, 6, 10)
    _, _, rec = _run_3d(hip, shape, True, _couplings("zero", shape, True), None, 2.0, "random")
    for k in ("n_clusters", "sum_size2", "sum_m2", "sum_m4"):
        assert [int(v) for v in rec[k]] == [240] * 3, k
    assert rec["largest"].tolist() == [1] * 3


@pytest.mark.parametrize("tile", [None, "2x2x2"])
def test_3d_everything_frozen(hip, monkeypatch, tile):
    """h = +10 along all-up spins at T = 0.5: every ghost bond's threshold is 2^32, every site hangs on the ghost."""
    if tile:
        monkeypatch.setenv("TSU_SW3D_TILE", tile)
    shape = (4, 6, 10)
    _, _, rec = _run_3d(hip, shape, True, _couplings("uniform", shape, True), _field("strong", shape), 0.5, "up")
    assert rec["n_frozen"].tolist() == rec["m_frozen"].tolist() == [240] * 3
    for k in ("n_clusters", "largest", "sum_size2", "sum_m2", "sum_m4"):
        assert [int(v) for v in rec[k]] == [0] * 3, k


# ---------------------------------------------------------------- batches and the switch
def _batch(hip, dim, mask, n_steps=3):
    """Four temperatures of 8 x 8 (dim 2) or 4 x 4 x 4 (dim 3) in one batch call, lattice i measured iff mask[i], against four
    lattices stepped one by one: (batch lattices' records, launch counts); spins and records compared here."""
    Ts, seeds = [1.8, 2.2, 2.6, 3.0] if dim == 2 else [3.5, 4.2, 4.9, 5.6], [SEED + i for i in range(4)]
    j = _couplings("uniform", (4, 4, 4), True)

    def make():
        lats = [hip.Lattice(8, 8, True) if dim == 2 else hip.Lattice3D(4, 4, 4, True) for _ in range(4)]
        for i, lat in enumerate(lats):
            lat.randomize(100 + i)
            if dim == 3:
                lat.set_disorder(*j)
            lat.cluster_measure(bool(mask[i]))
        return lats
    batch, single = make(), make()
    try:
        for step0 in (0, n_steps):
            if dim == 2:
                hip.cluster_sweep_batch(batch, n_steps, [1.0] * 4, Ts, seeds, [step0] * 4)
            else:
                hip.cluster_sweep_batch_3d(batch, n_steps, Ts, seeds, [step0] * 4)
            for i, lat in enumerate(single):
                lat.cluster_sweep(1.0, Ts[i], n_steps, seeds[i], step0) if dim == 2 else lat.cluster_sweep(Ts[i], n_steps, seeds[i], step0)
        recs = []
        for i in range(4):
            _same_spins(batch[i].get_spins(), single[i].get_spins(), f"batch lattice {i}")
            rb, rs = batch[i].cluster_record(), single[i].cluster_record()
            assert len(rb["n_clusters"]) == (n_steps if mask[i] else 0)
            for k in mtwin.FIELDS:
                assert list(rb[k]) == list(rs[k]), (i, k)
            recs.append(rb)
        return recs, [lat.cluster_launch_count() for lat in batch]
    finally:
        for lat in batch + single:
            lat.close()


@pytest.mark.parametrize("dim", [2, 3])
def test_measured_batch_equals_one_by_one(hip, dim):
    recs, launches = _batch(hip, dim, [1, 1, 1, 1])
    assert launches == [2] * 4  # one launch per batch call
    assert all((r["n_clusters"] > 0).all() for r in recs)
    assert len({tuple(r["n_clusters"]) for r in recs}) > 1  # every lattice has its own rows


@pytest.mark.parametrize("dim", [2, 3])
def test_batch_that_disagrees_on_the_switch(hip, dim):
    recs, _ = _batch(hip, dim, [1, 0, 1, 0])
    assert [len(r["n_clusters"]) for r in recs] == [3, 0, 3, 0]


def test_switching_off_restores_the_launch_count(hip, monkeypatch):
    monkeypatch.setenv("TSU_SW_TILE", "8")
    lat = hip.Lattice(24, 24, True)
    ref = hip.Lattice(24, 24, True)
    try:
        for x in (lat, ref):
            x.randomize(3)
        counts = []
        for on, step0 in ((False, 0), (True, 2), (False, 4)):
            lat.cluster_measure(on)
            before = lat.cluster_launch_count()
            lat.cluster_sweep(1.0, 2.3, 2, SEED, step0)
            counts.append(lat.cluster_launch_count() - before)
        ref.cluster_sweep(1.0, 2.3, 6, SEED, 0)
        assert counts == [6, 12, 6]
        _same_spins(lat.get_spins(), ref.get_spins(), "switch on and off")
        assert len(lat.cluster_record()["n_clusters"]) == 2  # the rows of the one measured call stay readable
    finally:
        lat.close()
        ref.close()


# ---------------------------------------------------------------- equilibrium against exact enumeration
def _batch_error(x, n_batches=20):
    x = np.asarray(x, dtype=np.float64)
    b = x[: len(x) // n_batches * n_batches].reshape(n_batches, -1).mean(axis=1)
    return float(b.std(ddof=1) / math.sqrt(n_batches))


def _exact_moments(n_sites, energies, T):
    """<M>, <M^2>, <M^4> of exp(-E / T) / Z from the energies of all 2^n states (bit i of the state's index = site i is up)."""
    k = np.arange(1 << n_sites)
    M = np.zeros(len(k))
    for i in range(n_sites):
        M += 2.0 * ((k >> i) & 1) - 1.0
    w = np.exp(-(energies - energies.min()) / T)
    w /= w.sum()
    return float(np.sum(w * M)), float(np.sum(w * M ** 2)), float(np.sum(w * M ** 4))


def _energies_3d(shape, d, n_sites):
    return np.array([lat3.energy(np.where((k >> np.arange(n_sites)) & 1, 1, -1).reshape(shape), False, *d) for k in range(1 << n_sites)])


def _energies_4x4_periodic():
    k = np.arange(1 << 16)
    s = np.stack([2 * ((k >> i) & 1) - 1 for i in range(16)], axis=1).reshape(-1, 4, 4)
    return -(np.sum(s * np.roll(s, -1, 1), axis=(1, 2)) + np.sum(s * np.roll(s, -1, 2), axis=(1, 2))).astype(np.float64)


# name: (shape, T, seed, disorder seed, ghost, thinning): the cases, seeds and thinning of test_cluster3d_gpu.test_exact_enumeration
# and test_cluster_field_gpu.test_exact_enumeration, and a 2-D 4 x 4 periodic ferromagnet at T_c
EQUILIBRIUM = {
    "2x2x2": ((2, 2, 2), 2.0, 11, 3, False, 4),
    "2x3x2": ((2, 3, 2), 1.5, 13, 5, False, 4),
    "2x2x2 ghost": ((2, 2, 2), 2.0, 11, 3, True, 4),
    "2x3x2 ghost": ((2, 3, 2), 1.5, 13, 5, True, 8),
    "4x4 periodic": ((4, 4), 2.269, 17, None, False, 4),
}
EQ_SAMPLES, EQ_BURN = 5000, 100


def equilibrium_deviations(name, rec):
    """{estimator: (mean, batch-means error, exact, deviation in errors)} of the thinned rows of `rec` (the dict of a record of
    EQ_SAMPLES * thinning steps) for the case `name`."""
    shape, T, _, dseed, ghost, every = EQUILIBRIUM[name]
    n_sites = int(np.prod(shape))
    if len(shape) == 2:
        E = _energies_4x4_periodic()
    else:
        d = lat3.enumeration_disorder(shape, dseed)
        E = _energies_3d(shape, d if ghost else d[:3], n_sites)
    m1, m2, m4 = _exact_moments(n_sites, E, T)
    s2 = np.array([int(v) for v in rec["sum_m2"]], dtype=object)[every - 1::every]
    s4 = np.array([int(v) for v in rec["sum_m4"]], dtype=object)[every - 1::every]
    mf = np.array([int(v) for v in rec["m_frozen"]], dtype=object)[every - 1::every]
    assert len(s2) == EQ_SAMPLES
    series = {"M2": ((s2 + mf * mf).astype(np.float64), m2)}
    if ghost:
        series["M"] = (mf.astype(np.float64), m1)
    else:
        series["M4"] = ((3 * s2 * s2 - 2 * s4).astype(np.float64), m4)
    out = {}
    for k, (x, exact) in series.items():
        err = _batch_error(x)
        out[k] = (float(np.mean(x)), err, exact, (float(np.mean(x)) - exact) / err)
    return out


@pytest.mark.parametrize("name", list(EQUILIBRIUM))
def test_improved_estimators_against_enumeration(hip, name):
    """<sum_m2 + m_frozen^2> against exact <M^2>; at zero field <3 sum_m2^2 - 2 sum_m4> against exact <M^4>; with a ghost <m_frozen>
    against exact <M>: 100 steps discarded, then the rows of 5000 steps taken every 4th (every 8th for 2 x 3 x 2 with a ghost, as in
    the tests these cases come from), 20 batch means, within 4 batch-means errors.  The rows are the twin's bit for bit (the tests
    above), so the outcome is the twin's, which gives at these seeds, in errors:
      2x2x2        M2 +1.73, M4 +1.45        2x3x2        M2 -1.23, M4 -1.22
      2x2x2 ghost  M2 +2.13, M  +0.25        2x3x2 ghost  M2 +1.23, M  -1.09
      4x4 periodic M2 +0.52, M4 +0.36"""
    shape, T, seed, dseed, ghost, every = EQUILIBRIUM[name]
    n = EQ_SAMPLES * every
    if len(shape) == 2:
        lat = hip.Lattice(*shape, True)
        sweep = lambda k, step0: lat.cluster_sweep(1.0, T, k, seed, step0)
    else:
        lat = hip.Lattice3D(*shape, False)
        d = lat3.enumeration_disorder(shape, dseed)
        lat.set_disorder(*(d if ghost else d[:3]))
        sweep = lambda k, step0: (lat.cluster_sweep_field if ghost else lat.cluster_sweep)(T, k, seed, step0)
    try:
        lat.fill(1)
        sweep(EQ_BURN, 0)
        lat.cluster_measure(True)
        sweep(n, EQ_BURN)
        rec = lat.cluster_record()
    finally:
        lat.close()
    for k, (mean, err, exact, dev) in equilibrium_deviations(name, rec).items():
        print(f"\n{name} {k}: {mean:.5f} +- {err:.5f}, exact {exact:.5f}, {dev:+.2f} errors")
        assert abs(dev) < 4.0, (name, k, mean, err, exact)


# ---------------------------------------------------------------- variance
def test_improved_m2_has_the_smaller_variance(hip):
    """Periodic 8^3, J = 1, T = 5.0, seed 3, 1500 steps, the first 200 dropped: the sample variance of sum_m2 against that of the
    plain M^2 of the same steps (the spins each step leaves).  sum_m2 is the mean of M^2 over the step's coins given its bonds
    (Rao-Blackwell), so the population variances are ordered; the twin, whose bits these are, gives the ratio 0.411 from an all-up start."""
    shape, T, seed = (8, 8, 8), 5.0, 3
    lat = hip.Lattice3D(*shape, True)
    try:
        lat.fill(1)
        lat.set_disorder(*_couplings("uniform", shape, True))
        lat.cluster_measure(True)
        improved, plain = [], []
        for t in range(1500):
            lat.cluster_sweep(T, 1, seed, t)
            improved.append(int(lat.cluster_record()["sum_m2"][0]))
            plain.append(int(lat.sum_spins()) ** 2)
    finally:
        lat.close()
    v_imp, v_plain = np.var(np.array(improved[200:], float), ddof=1), np.var(np.array(plain[200:], float), ddof=1)
    print(f"\nvariance ratio {v_imp / v_plain:.3f}")
    assert v_imp < v_plain


# ---------------------------------------------------------------- the scans
def test_scan_3d_improved_keys(hip):
    """temperature_scan_3d(improved=True): the new keys, all old keys bit-equal to the call without it, and chi_improved against the
    existing estimate where both are defined.  At zero field chi_improved = N <m^2> / T; the scan's `susceptibility` subtracts
    <|m|>^2, which `magnetization` gives back: N <m^2> / T = susceptibility + N magnetization^2 / T, the plain estimate from the 50
    measured |M|.  Their errors come from the same models stepped here again (same seeds, same bits): batch means of the 50 plain
    values (10 batches) and of the 500 rows (20 batches); at T = 5.0 the two agree within 4 combined errors."""
    from tsu.models import ising
    Ts = [4.0, 4.5, 5.0]
    kw = dict(size=8, temperatures=Ts, algorithm="swendsen_wang")
    plain = ising.temperature_scan_3d(**kw)
    imp = ising.temperature_scan_3d(improved=True, **kw)
    new = {"m2_improved", "chi_improved", "binder_improved", "mean_cluster_size", "largest_cluster", "n_clusters"}
    assert set(imp) == set(plain) | new and "m_improved" not in imp
    for k in plain:
        assert np.asarray(imp[k]).tobytes() == np.asarray(plain[k]).tobytes(), k
    for k in new:
        assert imp[k].shape == (3,) and np.isfinite(imp[k]).all(), k
    N = 512
    assert (imp["largest_cluster"] <= 1).all() and (imp["n_clusters"] >= 1).all() and (imp["mean_cluster_size"] >= 1).all()
    assert (np.diff(imp["m2_improved"]) < 0).all()  # <m^2> falls with T across the transition
    assert np.allclose(imp["chi_improved"], N * imp["m2_improved"] / np.array(Ts), rtol=1e-15)
    # T = 5.0 again, by hand: model 2 of the scan (seed 0 + 2, all up, 1000 steps, then 50 x 10 measured steps)
    m = ising.IsingModel3D(8, temperature=5.0, seed=2, initial="up")
    m.cluster_update(1000)
    rows, Ms = [], []
    for _ in range(50):
        m.cluster_update(10, measure=True)
        rows.append(ising.cluster_estimators(m.cluster_record())["m2"])
        Ms.append(m.magnetization())
    rows, Ms = np.concatenate(rows), np.array(Ms)
    assert float(np.mean(rows)) == imp["m2_improved"][2]
    chi_plain = imp["susceptibility"][2] + N * imp["magnetization"][2] ** 2 / 5.0
    assert math.isclose(chi_plain, N * float(np.mean(Ms ** 2)) / 5.0, rel_tol=1e-12)
    e_plain, e_imp = N * _batch_error(Ms ** 2, 10) / 5.0, N * _batch_error(rows, 20) / 5.0
    print(f"\nchi plain {chi_plain:.4f} +- {e_plain:.4f}, improved {imp['chi_improved'][2]:.4f} +- {e_imp:.4f}")
    assert abs(imp["chi_improved"][2] - chi_plain) < 4 * math.hypot(e_plain, e_imp)


def test_scan_ghost_and_2d_improved_keys(hip):
    from tsu.models import ising
    g = ising.temperature_scan_3d(4, [4.0, 5.0], algorithm="swendsen_wang_ghost", external_field=0.05, n_equilibrate=50, n_measure=5,
                                  measure_every=4, improved=True)
    assert "m_improved" in g and "binder_improved" not in g and (g["m_improved"] > 0).all()
    assert np.allclose(g["chi_improved"], 64 * (g["m2_improved"] - g["m_improved"] ** 2) / g["temperatures"], rtol=1e-12)
    kw = dict(size=8, temperatures=[2.0, 2.5], algorithm="swendsen_wang", n_equilibrate=50, n_measure=5, measure_every=4)
    p, i2 = ising.temperature_scan(**kw), ising.temperature_scan(improved=True, **kw)
    for k in p:
        assert np.asarray(i2[k]).tobytes() == np.asarray(p[k]).tobytes(), k
    assert {"m2_improved", "chi_improved", "binder_improved", "mean_cluster_size", "largest_cluster", "n_clusters"} <= set(i2)
    assert (i2["binder_improved"] > 0).all() and (i2["binder_improved"] <= 1).all()

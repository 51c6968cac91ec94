"""The far end of every GPU path's inputs (-m gpu): full-width seeds, replica ids up to 2^24 - 1, counters at the top of their
range, and the strip renumbering of the tile-resident lattice kernel.  The other parity tests start where a run starts (a seed below
2^16, counters of a few hundred, replica ids 0 .. 10, a fresh handle); a kernel that dropped seed >> 32, cut the replica id, or
computed a half-sweep counter in a signed int would pass all of them.  tests/helpers/far_end.py holds the one table of inputs.

Every case is bit-exact against the C oracle or the NumPy twin of its kernel, never against another GPU route alone, and asserts its
route by launch count or plan where the route tests do.  The entry points' limits (sweep0 + n <= 2^31 for lattice sweeps, 2^32 for
cluster steps, dense and sparse sweeps, replica < 2^24) are pinned from both sides: at the limit the call runs and is exact, one
past it the call is refused, launches nothing and leaves the state as it was."""
import functools
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as ora

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fe = _load("far_end")
k7 = _load("disorder_twin")
k8 = _load("lattice3d_twin")
sw2 = _load("cluster_twin")
sw3 = _load("cluster3d_twin")
swf = _load("cluster_field_twin")
plans = _load("sparse_plan_twin")
ovl = _load("overlap_twin")
cor = _load("correlation_twin")

SEED = fe.SEED_HI
REP = fe.REPLICA_MAX
T_C = 2.269185
GEN_LIMIT = 16383  # strip generations are numbered 1 .. 16382 (14-bit tags of the byte planes)


@pytest.fixture(scope="module")
def hip():
    from tsu import _hip
    _hip.Context.default()
    return _hip


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in ("TSU_SW_TILE", "TSU_SW3D_TILE", "TSU_K5_PAIR", "TSU_K5_TEST_TIE", "TSU_K5_STENCIL", "TSU_K5_V4", "TSU_K2_OWN_TEST_FAIL"):
        monkeypatch.delenv(k, raising=False)


def _same(got, want, what):
    assert (got == want).all(), f"{what}: differs at {np.argwhere(got != want)[:5].tolist()} ({int((got != want).sum())} sites)"


def _child(case, env):
    r = subprocess.run([sys.executable, os.path.join(HERE, "helpers", "far_end_check.py"), json.dumps(case)],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


# =================================================================================================== K1

TABLE = functools.lru_cache(maxsize=None)(lambda: ora.ising2d_thresholds(1.0, 0.05, T_C, 0))

# (rows, cols, periodic, kernel, sweeps per launch, launches a call of 19 sweeps may make)
#   k1_planes: one launch per call; k1_generic: one per colour; the tiled kernel at 8 sweeps per launch: at most ceil(19 / 8), and one
#   when the tiles stay resident; k1_resident (library's choice above 8 sweeps per call): one
K1_CASES = [
    (30, 48, True, "auto", 0, (1,)), (33, 47, False, "auto", 0, (1,)),
    (1, 9, False, "auto", 0, (38,)),
    (130, 300, True, "tiled", 8, (1, 3)), (96, 290, False, "tiled", 8, (1, 3)), (128, 1024, True, "tiled", 8, (1, 3)),
    (1024, 1024, True, "auto", 0, (1,)), (1000, 1000, True, "auto", 0, (1,)), (1000, 1000, False, "tiled", 0, (1,)),
]


@pytest.mark.parametrize("rows,cols,periodic,kernel,spl,launches", K1_CASES)
def test_k1_routes(hip, rows, cols, periodic, kernel, spl, launches):
    """SEED_HI, replica 2^24 - 1, two calls of 19 sweeps on one handle: across sweep 2^30 (hs crosses 2^31), then up to the limit (the
    last half-sweep is hs = 2^32 - 1).  19 sweeps are several generations and a short last one on the tiled kernels."""
    table = TABLE()
    lat = hip.Lattice(rows, cols, periodic)
    try:
        lat.set_kernel({"auto": hip.KERNEL_AUTO, "tiled": hip.KERNEL_TILED}[kernel], spl)
        lat.randomize(SEED, fe.REPLICA_BYTES)
        want = ora.ising2d_randomize(rows, cols, SEED, fe.REPLICA_BYTES)
        _same(lat.get_spins(), want, "randomize")
        lat.set_thresholds(table)
        for name, sweep0 in fe.lattice_positions(19):
            n0 = lat.launch_count()
            lat.sweep(19, SEED, sweep0, REP)
            got_launches = lat.launch_count() - n0
            want = ora.ising2d_sweep(want, periodic, table, 19, SEED, sweep0, REP)
            _same(lat.get_spins(), want, f"{rows}x{cols} {name}")
            assert lat.observables() == ora.ising2d_observables(want, periodic)
            assert got_launches in launches, f"{name}: {got_launches} launches"
    finally:
        lat.close()


def test_k1_nibble_planes(hip):
    """Nibble colour planes forced on 1024 x 1024 (512 x 512 tiles, tile-resident), as tests/test_nibble_gpu.py forces them."""
    for periodic in (1, 0):
        out = _child({"mode": "sweeps", "rows": 1024, "cols": 1024, "periodic": periodic, "k": 8, "seed": SEED, "replica": REP,
                      "calls": [[s0, 19] for _, s0 in fe.lattice_positions(19)]}, {"TSU_TILE_VARIANT": "8"})
        assert out.count("ok 1024x1024") == 2


def test_k1_sample(hip):
    """tsu_ising2d_sample on 130 x 36: burn-in 4, then 3 samples 5 sweeps apart, the run ending at the limit."""
    rows, cols, burn, ns, m = 130, 36, 4, 5, 3
    table = TABLE()
    sweep0 = fe.end(burn + m * ns)
    lat = hip.Lattice(rows, cols, True)
    try:
        lat.randomize(SEED, REP)
        lat.set_thresholds(table)
        got = lat.sample(burn, ns, m, SEED, sweep0, fe.REPLICA_BYTES)
        cur = ora.ising2d_sweep(ora.ising2d_randomize(rows, cols, SEED, REP), True, table, burn, SEED, sweep0, fe.REPLICA_BYTES)
        for k in range(m):
            cur = ora.ising2d_sweep(cur, True, table, ns, SEED, sweep0 + burn + k * ns, fe.REPLICA_BYTES)
            _same(got[k], cur, f"sample {k}")
        _same(lat.get_spins(), cur, "resident state")
    finally:
        lat.close()


@pytest.mark.parametrize("rows,cols", [(32, 32), (128, 1024)])
def test_k1_sweep_batch(hip, rows, cols):
    """tsu_ising2d_sweep_batch with per-lattice seeds, counters and replica ids from the table: one launch of the one-workgroup kernel
    (32 x 32), side streams of the tiled kernel (128 x 1024)."""
    n = 9
    seeds = [SEED, fe.SEED_CARRY, SEED ^ 0xFFFFFFFF, fe.SEED_CARRY + 5]
    sweep0s = [fe.end(n), fe.straddle(n), fe.end(n) - 1, 2 ** 30 - 1]
    reps = [REP, fe.REPLICA_BYTES, 0, REP - 1]
    lats, want = [], []
    for i in range(4):
        lat = hip.Lattice(rows, cols, True)
        lat.randomize(seeds[i], reps[i])
        lat.set_model(1.0, 0.05 * i, 2.0 + 0.3 * i)
        lats.append(lat)
        table = ora.ising2d_thresholds(1.0, 0.05 * i, 2.0 + 0.3 * i, 0)
        want.append(ora.ising2d_sweep(ora.ising2d_randomize(rows, cols, seeds[i], reps[i]), True, table, n, seeds[i], sweep0s[i], reps[i]))
    n0 = [lat.launch_count() for lat in lats]
    hip.sweep_batch(lats, n, seeds, sweep0s, reps)
    for i, lat in enumerate(lats):
        _same(lat.get_spins(), want[i], f"lattice {i}")
        if rows == 32:
            assert lat.launch_count() - n0[i] == 1
        lat.close()


def test_k1_two_slabs(hip):
    """Two 128 x 576 slabs with 8 ghost rows (the scheme of test_ising2d_tiled_slabs), refresh periods of 4 sweeps across sweep 2^30."""
    per, cols, ghost, k, nslab = 128, 576, 8, 4, 2
    rows = per * nslab
    table = TABLE()
    want = ora.ising2d_randomize(rows, cols, SEED, REP)
    slabs = [hip.Lattice(per, cols, True, total_rows=rows, row0=i * per, ghost=ghost) for i in range(nslab)]
    try:
        for i, s in enumerate(slabs):
            s.set_kernel(hip.KERNEL_TILED, 0)
            s.set_spins(want[i * per:(i + 1) * per])
            s.set_thresholds(table)
        for it in range(3):
            sweep0 = fe.straddle(3 * k) + it * k
            owned = [s.get_spins() for s in slabs]
            for i, s in enumerate(slabs):
                s.set_spins(owned[(i - 1) % nslab][-ghost:], row_first=-ghost)
                s.set_spins(owned[(i + 1) % nslab][:ghost], row_first=per)
            for s in slabs:
                s.sweep(k, SEED, sweep0, REP)
            want = ora.ising2d_sweep(want, True, table, k, SEED, sweep0, REP)
            _same(np.concatenate([s.get_spins() for s in slabs]), want, f"period {it}")
    finally:
        for s in slabs:
            s.close()


# =================================================================================================== K2

def _dense_system(n, f64, seed):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n)).astype(np.float32)
    J = ((G + G.T) / 2 / np.sqrt(n)).astype(np.float32)
    np.fill_diagonal(J, 0.0)
    b = rng.normal(size=n) * 0.1
    return (J.astype(np.float64) if f64 else J), b, rng.integers(0, 2, size=n).astype(np.int8)


# (n, fp64 couplings, caller's order, route); tsu_dense_launch_counts counts k2_own and k2_pipe launches: "none" is neither
K2_CASES = [
    (12, False, False, "none"), (192, False, False, "none"),        # k2_small: one wave
    (200, False, False, "none"), (448, True, False, "none"),        # k2_wg: one workgroup
    (580, False, False, "pipe"),                                    # k2_pipe
    (2051, True, False, "none"),                                    # the cooperative kernel (not a multiple of 4)
    (2048, False, False, "own"), (4100, True, False, "own"),        # k2_own: one launch per call
    (2048, False, True, "own"), (4100, True, True, "own"),          # ... with a caller's order
]


@pytest.mark.parametrize("n,f64,ordered,route", K2_CASES)
def test_k2_routes(hip, n, f64, ordered, route):
    """5 sweeps with SEED_HI across sweep 2^31, then 5 ending at 2^32 (the last sweep counter is 2^32 - 1)."""
    J, b, st = _dense_system(n, f64, n)
    J64 = np.asarray(J, dtype=np.float64)
    d = hip.DenseSystem(J, b, hip.DTYPE_F64 if f64 else hip.DTYPE_F32)
    try:
        d.set_state(st)
        want = st
        rng = np.random.default_rng(n + 1)
        for (name, sweep0), rep in zip(fe.counter_positions(5), fe.REPLICAS):
            order = np.array([rng.permutation(n) for _ in range(5)]) if ordered else None
            d.sweep(0.9, 5, seed=SEED, sweep0=sweep0, replica=rep, order=order)
            want = ora.dense_sweep_philox(want, J64, b, 0.9, 5, SEED, sweep0=sweep0, replica=rep, order=order)
            _same(d.get_state(), want, f"n={n} {name}")
        own, pipe = d.launch_counts()
        assert (own, pipe) == (0, 0) if route == "none" else (own == 0 and pipe >= 2) if route == "pipe" else own == 2, (own, pipe)
    finally:
        d.close()


def test_k2_own_replicas(hip):
    """k2_own with three replicas in one launch: per-replica seeds, counters and replica ids at the far end."""
    n, R, ns = 2304, 3, 5
    J, b, _ = _dense_system(n, False, 3 * n)
    J64 = J.astype(np.float64)
    sts = np.array([np.random.default_rng(100 + r).integers(0, 2, size=n) for r in range(R)], dtype=np.int8)
    temps = [0.8, 1.0, 1.3]
    seeds = [SEED, fe.SEED_CARRY, fe.SEED_CARRY + 3]
    sw0 = [fe.end32(ns), fe.straddle32(ns), fe.end32(ns) - 1]
    reps = [REP, fe.REPLICA_BYTES, REP - 1]
    d = hip.DenseSystem(J, b, hip.DTYPE_F32)
    try:
        out = d.sweep_replicas(sts, temps, ns, seeds, sw0, replicas=reps)
        assert d.launch_counts()[0] == 1
        for r in range(R):
            want = ora.dense_sweep_philox(sts[r], J64, b, temps[r], ns, seeds[r], sweep0=sw0[r], replica=reps[r])
            _same(out[r], want, f"replica {r}")
    finally:
        d.close()


@pytest.mark.parametrize("n", [150, 600])
def test_k2_sample_and_anneal(hip, n):
    """A sampling run across sweep 2^31 and an annealing schedule ending at 2^32 (one wave / one workgroup at 150, k2_pipe at 600)."""
    J, b, st = _dense_system(n, False, 7 * n)
    J64 = J.astype(np.float64)
    burn, ns, m = 2, 2, 3
    d = hip.DenseSystem(J, b, hip.DTYPE_F32)
    try:
        d.set_state(st)
        sweep0 = 2 ** 31 - 3
        got = d.sample(0.8, burn, ns, m, seed=SEED, sweep0=sweep0, replica=REP)
        cur = ora.dense_sweep_philox(st, J64, b, 0.8, burn, SEED, sweep0=sweep0, replica=REP)
        for k in range(m):
            cur = ora.dense_sweep_philox(cur, J64, b, 0.8, ns, SEED, sweep0=sweep0 + burn + k * ns, replica=REP)
            _same(got[k], cur, f"sample {k}")
        temps = 3.0 * (0.1 / 3.0) ** (np.arange(6) / 6.0)
        sweep0 = fe.end32(temps.size)
        got = d.anneal(temps, seed=SEED, sweep0=sweep0, replica=fe.REPLICA_BYTES)
        for k, T in enumerate(temps):
            cur = ora.dense_sweep_philox(cur, J64, b, float(T), 1, SEED, sweep0=sweep0 + k, replica=fe.REPLICA_BYTES)
            _same(got[k], cur, f"anneal step {k}")
        _same(d.get_state(), cur, "resident state")
    finally:
        d.close()


# =================================================================================================== K5

# one case per route of tests/test_sparse_routes_gpu.py's table at its smallest n, the chain's paired classes, and k5_small
K5_CASES = ([(g, 40008) for g in ("dimers", "degree3", "degree4", "asymmetric", "halves", "chain", "chain_first38", "chain_first64",
                                  "chain_first65", "chain_both_ends", "chain_interior", "chain_descending")]
            + [("chain_odd_first", 40009), ("strip", 30000), ("strip", 60000), ("chain", 4099)])


@functools.lru_cache(maxsize=None)
def _graph(name, n):
    return plans.graph(name, n)


@pytest.mark.parametrize("name,n", K5_CASES)
def test_k5_routes(hip, name, n):
    A, bias, offsets, order, classes, pairs = _graph(name, n)
    g = hip.SparseSystem(A.indptr, A.indices, A.data, bias, offsets, order)
    try:
        plan = g.plan()
        if n <= 32768:
            assert {r["route"] for r in plan} == {2}
        else:
            assert plan == plans.expected_plan(offsets, classes, pairs)
        if name == "chain" and n > 32768:
            assert [(r["route"], r["pair"]) for r in plan] == [(1, 1), (1, 2)]
        want = np.random.default_rng(n).integers(0, 2, size=n).astype(np.int8)
        g.set_state(want)
        for (pname, sweep0), rep in zip(fe.counter_positions(5), fe.REPLICAS):
            g.sweep(1.1, 5, seed=SEED, sweep0=sweep0, replica=rep)
            want = ora.sparse_sweep_philox(want, A.indptr, A.indices, A.data, bias, 1.1, 5, SEED, sweep0=sweep0, replica=rep, order=order)
            _same(g.get_state(), want, f"{name} {n} {pname}")
        sweep0 = fe.end32(3)
        got = g.sample(0.7, 1, 1, 2, seed=fe.SEED_CARRY, sweep0=sweep0, replica=REP)
        for k in range(2):
            want = ora.sparse_sweep_philox(want, A.indptr, A.indices, A.data, bias, 0.7, 2 - k, fe.SEED_CARRY, sweep0=sweep0 + 2 * k,
                                           replica=REP, order=order)
            _same(got[k], want, f"{name} {n} sample {k}")
    finally:
        g.close()


# =================================================================================================== K7, K8 sweeps

def _gauss2d(rows, cols, periodic, dseed):
    rng = np.random.default_rng(dseed)
    jr, jd, h = (rng.normal(size=(rows, cols)).astype(np.float32) for _ in range(3))
    if not periodic:
        jr[:, -1] = 0.0
        jd[-1, :] = 0.0
    return jr, jd, h


def _gauss3d(shape, periodic, dseed, field=True):
    rng = np.random.default_rng(dseed)
    jr, jd, jl, h = (rng.normal(size=shape).astype(np.float32) for _ in range(4))
    pz, pr, pc = k8.axes(periodic)
    if not pc:
        jr[:, :, -1] = 0.0
    if not pr:
        jd[:, -1, :] = 0.0
    if not pz:
        jl[-1, :, :] = 0.0
    return jr, jd, jl, (h if field else None)


@pytest.mark.parametrize("rows,cols,periodic", [(37, 53, False), (64, 64, True)])
def test_k7_sweeps(hip, rows, cols, periodic):
    jr, jd, h = _gauss2d(rows, cols, periodic, 5)
    a, b = hip.Lattice(rows, cols, periodic), hip.Lattice(rows, cols, periodic)
    try:
        for lat in (a, b):
            lat.set_disorder(jr, jd, h)
        a.randomize(SEED, REP)
        b.randomize(fe.SEED_CARRY, fe.REPLICA_BYTES)
        wa = ora.ising2d_randomize(rows, cols, SEED, REP)
        wb = ora.ising2d_randomize(rows, cols, fe.SEED_CARRY, fe.REPLICA_BYTES)
        for name, sweep0 in fe.lattice_positions(5):
            n0 = a.disorder_launch_count()
            a.disorder_sweep(1.3, 5, SEED, sweep0, REP)
            b.disorder_sweep(1.3, 5, fe.SEED_CARRY, sweep0, fe.REPLICA_BYTES)
            assert a.disorder_launch_count() - n0 == 10
            wa = k7.sweep(wa, periodic, jr, jd, h, 1.3, 5, SEED, sweep0, REP)
            wb = k7.sweep(wb, periodic, jr, jd, h, 1.3, 5, fe.SEED_CARRY, sweep0, fe.REPLICA_BYTES)
            _same(a.get_spins(), wa, f"{name} a")
            _same(b.get_spins(), wb, f"{name} b")
            assert a.disorder_energy() == pytest.approx(k7.energy(wa, periodic, jr, jd, h), rel=1e-12)
            assert a.overlap(b) == k7.overlap(wa, wb)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("shape,periodic", [((3, 5, 37), False), ((8, 6, 40), (True, False, True))])
def test_k8_sweeps(hip, shape, periodic):
    jr, jd, jl, h = _gauss3d(shape, periodic, 6)
    a, b = hip.Lattice3D(*shape, periodic), hip.Lattice3D(*shape, periodic)
    try:
        for lat in (a, b):
            lat.set_disorder(jr, jd, jl, h)
        a.randomize(SEED, REP)
        b.randomize(fe.SEED_CARRY, fe.REPLICA_BYTES)
        rows2d = shape[0] * shape[1]
        wa = ora.ising2d_randomize(rows2d, shape[2], SEED, REP).reshape(shape)
        wb = ora.ising2d_randomize(rows2d, shape[2], fe.SEED_CARRY, fe.REPLICA_BYTES).reshape(shape)
        _same(a.get_spins(), wa, "randomize")
        for name, sweep0 in fe.lattice_positions(5):
            n0 = a.launch_count()
            a.sweep(1.3, 5, SEED, sweep0, REP)
            b.sweep(1.3, 5, fe.SEED_CARRY, sweep0, fe.REPLICA_BYTES)
            assert a.launch_count() - n0 == 10
            wa = k8.sweep(wa, periodic, jr, jd, jl, h, 1.3, 5, SEED, sweep0, REP)
            wb = k8.sweep(wb, periodic, jr, jd, jl, h, 1.3, 5, fe.SEED_CARRY, sweep0, fe.REPLICA_BYTES)
            _same(a.get_spins(), wa, f"{name} a")
            _same(b.get_spins(), wb, f"{name} b")
            assert a.energy() == pytest.approx(k8.energy(wa, periodic, jr, jd, jl, h), rel=1e-12)
            assert a.overlap(b) == k8.overlap(wa, wb)
    finally:
        a.close()
        b.close()


# =================================================================================================== cluster steps (K6, K8, ghost)

@pytest.mark.parametrize("rows,cols,edge", [(37, 53, None), (130, 70, 16)])
def test_k6_cluster_steps(hip, monkeypatch, rows, cols, edge):
    """4 steps across step 2^31, then 4 ending at 2^32: the one-workgroup route (one launch per call) and, with the tile-edge knob,
    the tiled route (three launches per step)."""
    if edge:
        monkeypatch.setenv("TSU_SW_TILE", str(edge))
    lat = hip.Lattice(rows, cols, False)
    try:
        lat.randomize(SEED, REP)
        want = ora.ising2d_randomize(rows, cols, SEED, REP)
        for (name, step0), rep in zip(fe.counter_positions(4), fe.REPLICAS):
            n0 = lat.cluster_launch_count()
            lat.cluster_sweep(1.0, T_C, 4, SEED, step0, rep)
            assert lat.cluster_launch_count() - n0 == (12 if edge else 1)
            want = sw2.sweep(want, False, 1.0, T_C, 4, SEED, step0, rep)
            _same(lat.get_spins(), want, f"{rows}x{cols} {name}")
    finally:
        lat.close()


@pytest.mark.parametrize("ghost", [False, True])
@pytest.mark.parametrize("shape,periodic,tile", [((4, 6, 8), False, None), ((8, 8, 16), True, "3x5x6")])
def test_k8_cluster_steps(hip, monkeypatch, shape, periodic, tile, ghost):
    """The same two calls on the 3-D handle, zero-field steps and ghost-spin steps in a Gaussian field, both routes."""
    if tile:
        monkeypatch.setenv("TSU_SW3D_TILE", tile)
    jr, jd, jl, h = _gauss3d(shape, periodic, 7, field=ghost)
    lat = hip.Lattice3D(*shape, periodic)
    try:
        lat.randomize(SEED, REP)
        lat.set_disorder(jr, jd, jl, h)
        want = lat.get_spins()
        _same(want, ora.ising2d_randomize(shape[0] * shape[1], shape[2], SEED, REP).reshape(shape), "randomize")
        for (name, step0), rep in zip(fe.counter_positions(4), fe.REPLICAS):
            n0 = lat.cluster_launch_count()
            if ghost:
                lat.cluster_sweep_field(1.2, 4, SEED, step0, rep)
                want = swf.sweep(want, periodic, jr, jd, jl, h, 1.2, 4, SEED, step0, rep)
            else:
                lat.cluster_sweep(1.2, 4, SEED, step0, rep)
                want = sw3.sweep(want, periodic, jr, jd, jl, 1.2, 4, SEED, step0, rep)
            assert lat.cluster_launch_count() - n0 == (12 if tile else 1)
            _same(lat.get_spins(), want, f"{shape} {name}")
    finally:
        lat.close()


# =================================================================================================== handles with internal counters

def _by_walker(hist, R):
    def energies(j, k):
        E = np.empty(R)
        E[hist["walker"][j, k]] = hist["E"][j, k]
        return E
    return energies


# SEED_HI, and a SEED_CARRY-style seed: walker keys are seed + k n_temps + w, so 2^32 - 4 puts the carry into the high key word at
# walker 4 of ladder 0 (five temperatures) and the whole of ladder 1 above it
LADDER_SEEDS = [SEED, 2 ** 32 - 4]


@pytest.mark.parametrize("seed", LADDER_SEEDS)
def test_pt2d_ladders(hip, monkeypatch, seed):
    """tsu_pt2d on 9 x 12 open, 5 temperatures, 2 ladders, a replica cluster pass every round, link overlap recorded: the start is
    the oracle's randomize(seed + index), the run is the ladder twin fed the device's energies."""
    monkeypatch.delenv("TSU_ICM_TILE", raising=False)
    icm = _load("icm_twin")
    rows, cols, periodic, R = 9, 12, False, 5
    Ts = list(np.linspace(0.4, 2.0, R))
    dis = _gauss2d(rows, cols, periodic, 11)
    pt = hip.TemperingLattice(rows, cols, periodic, R, 2)
    try:
        pt.set_disorder(*dis)
        pt.set_temperatures(Ts)
        pt.set_cluster_moves(1, float("inf"))
        pt.set_link_overlap(True)
        pt.init(seed)
        start = [[pt.get_spins(k, w) for w in range(R)] for k in range(2)]
        for k in range(2):
            for w in range(R):
                _same(start[k][w], ora.ising2d_randomize(rows, cols, seed + k * R + w), f"start of walker {w} of ladder {k}")
        tw = icm.Ladders(start, periodic, dis, Ts, seed, 1, float("inf"))
        for n_rounds, interval in ((4, 2), (3, 1)):
            pt.run(n_rounds, interval, swap=True, record=True)
            hist = pt.history()
            want = tw.run(n_rounds, interval, True, True, _by_walker(hist, R))
            for key in ("walker", "M", "q"):
                assert (hist[key] == want[key]).all(), key
            st = pt.stats()
            assert (st["attempts"] == tw.attempts).all() and (st["accepts"] == tw.accepts).all()
            assert (st["walker_at_slot"] == tw.walker_at_slot).all() and (st["round_trips"] == tw.trips).all()
            assert st["sweep_count"] == tw.sweeps and st["round_count"] == tw.rounds
        E, _ = pt.energies()
        for i in range(R):
            a, b = (tw.spins[k][tw.walker_at_slot[k, i]] for k in range(2))
            for k, s in enumerate((a, b)):
                _same(pt.get_spins(k, i), s, f"slot {i} ladder {k}")
                assert E[k, tw.walker_at_slot[k, i]] == pytest.approx(k7.energy(s, periodic, *dis), rel=1e-12, abs=1e-9)
            assert hist["q_link"][-1, i] == ovl.link_overlap(a, b, periodic)[0]
            for got, ref in zip(pt.profiles(i), cor.profiles(a, b)):
                assert (got == ref).all()
        cs = pt.cluster_stats()
        assert cs["pass_count"] == tw.passes == 7 and (cs["clusters"] == tw.clusters).all() and (cs["flipped"] == tw.flipped).all()
        assert tw.accepts.sum() > 0 and tw.flipped.sum() > 0
    finally:
        pt.close()


@pytest.mark.parametrize("seed", LADDER_SEEDS)
def test_pt3d_ladders(hip, seed):
    """tsu_pt3d on (3, 5, 9) open, 5 temperatures, 2 ladders, link overlap recorded, against tests/helpers/tempering3d_twin.py."""
    t3 = _load("tempering3d_twin")
    shape, periodic, R = (3, 5, 9), False, 5
    Ts = list(np.linspace(0.5, 2.5, R))
    dis = _gauss3d(shape, periodic, 12)
    pt = hip.TemperingLattice3D(*shape, periodic, R, 2)
    try:
        pt.set_disorder(*dis)
        pt.set_temperatures(Ts)
        pt.set_link_overlap(True)
        pt.init(seed)
        start = [[pt.get_spins(k, w) for w in range(R)] for k in range(2)]
        ref = t3.initial_spins(shape, seed, 2 * R)
        for k in range(2):
            for w in range(R):
                _same(start[k][w], ref[k * R + w], f"start of walker {w} of ladder {k}")
                _same(ref[k * R + w], ora.ising2d_randomize(shape[0] * shape[1], shape[2], seed + k * R + w).reshape(shape), "twin start")
        tw = t3.Ladders(start, periodic, dis, Ts, seed)
        pt.run(4, 2, swap=True, record=True)
        hist = pt.history()
        want = tw.run(4, 2, True, True, _by_walker(hist, R))
        for key in ("walker", "M", "q"):
            assert (hist[key] == want[key]).all(), key
        st = pt.stats()
        assert (st["attempts"] == tw.attempts).all() and (st["accepts"] == tw.accepts).all() and tw.accepts.sum() > 0
        assert st["sweep_count"] == tw.sweeps == 8 and st["round_count"] == tw.rounds == 4
        E, _ = pt.energies()
        for i in range(R):
            a, b = (tw.spins[k][tw.walker_at_slot[k, i]] for k in range(2))
            for k, s in enumerate((a, b)):
                _same(pt.get_spins(k, i), s, f"slot {i} ladder {k}")
                assert E[k, tw.walker_at_slot[k, i]] == pytest.approx(k8.energy(s, periodic, *dis), rel=1e-12, abs=1e-9)
            assert hist["q_link"][-1, i] == ovl.link_overlap(a, b, periodic)[0]
            for got, ref_p in zip(pt.profiles(i), cor.profiles(a, b)):
                assert (got == ref_p).all()
    finally:
        pt.close()


@pytest.mark.parametrize("route", ["small", "colour"])
@pytest.mark.parametrize("seed", [SEED, fe.SEED_CARRY + 2])
def test_sparse_batch_ladders(hip, monkeypatch, route, seed):
    """tsu_sparse_batch on a 200-site random graph, both routes: the contract's random start, then 6 rounds of 3 sweeps of 2 ladders of 5
    walkers against tests/helpers/sparse_batch_twin.py fed the device's energies.  (Walker g has replica id g and the handle's seed.)"""
    from test_sparse_cpu import random_graph  # (tests/ is on sys.path: rootdir conftest, prepend import mode)
    from tsu.models import GraphTempering
    sb = _load("sparse_batch_twin")
    if route == "colour":
        monkeypatch.setenv("TSU_K5B_SMALL", "0")
    else:
        monkeypatch.delenv("TSU_K5B_SMALL", raising=False)
    A = random_graph(200, 0.03, 200)
    bias = np.random.default_rng(200).normal(size=200)
    temps = [0.7, 1.0, 1.4, 2.0, 2.9]
    with GraphTempering(A, temps, bias=bias, ladders=2, seed=seed) as pt:
        assert pt.plan()["route"] == route
        for g in range(10):
            _same(pt.state(g % 5, ladder=g // 5), sb.random_start(200, g, seed), f"random start of walker {g}")
        pt.run(6, 3)
        hist = [pt.history(ladder=k) for k in range(2)]
        E, M, W = (np.stack([h[key] for h in hist], axis=1) for key in ("E", "M", "walker"))
        E_walker = np.empty_like(E)
        np.put_along_axis(E_walker, W.astype(np.int64), E, axis=-1)
        b = sb.Batch(A, bias, pt.order, temps, ladders=2, seed=seed)
        tE, tM, tW = b.run(6, 3, energies=lambda j, _b: E_walker[j].reshape(-1))
        _same(W, tW, "walker")
        _same(M, tM, "M")
        _same(E, tE, "E")
        attempts, accepts = pt.swap_counts()
        _same(attempts, b.attempts, "attempts")
        _same(accepts, b.accepts, "accepts")
        assert accepts.sum() > 0 and pt.sweep_count == 18 == b.sweeps
        for k in range(2):
            for i in range(5):
                _same(pt.state(i, ladder=k), b.state_at(i, ladder=k), f"slot {i} ladder {k}")


# =================================================================================================== K3

@pytest.mark.parametrize("n_chains,dim", [(3, 64), (2, 1027)])
def test_k3_separable(hip, n_chains, dim):
    """SEED_HI through the separable kernel and the restart, at the tolerance of test_langevin_matches_oracle (2e-4 absolute)."""
    rng = np.random.default_rng(dim)
    x = rng.normal(size=(n_chains, dim)).astype(np.float32)
    k = rng.uniform(0.5, 2.0, size=dim).astype(np.float32)
    mu = rng.normal(size=dim).astype(np.float32)
    lc = hip.LangevinChains(n_chains, dim)
    try:
        lc.set_energy(k, mu)
        lc.set_state(x)
        traj = lc.step(20, 0.02, 1.5, 0.7, SEED, step0=3, chain0=5, trajectory=True)
        want, wtraj = ora.langevin_quadratic_f32(x, k, mu, 20, 0.02, 1.5, 0.7, SEED, step0=3, chain0=5, trajectory=True)
        np.testing.assert_allclose(traj, wtraj, rtol=0, atol=2e-4)
        np.testing.assert_allclose(lc.get_state(), want, rtol=0, atol=2e-4)
        lc.restart(mu, 0.1, SEED, chain0=2)
        wantr = np.array([[mu[i] + np.float32(0.1) * ora.langevin_normals_f32(i >> 2, 2 + c, 0, SEED, ora.TAG_LANGEVIN_RESTART)[i & 3]
                           for i in range(dim)] for c in range(n_chains)], dtype=np.float32)
        np.testing.assert_allclose(lc.get_state(), wantr, rtol=0, atol=2e-4)
    finally:
        lc.close()


@pytest.mark.parametrize("d,chains", [(64, 3), (1500, 9)])
def test_k3_coupled(hip, d, chains):
    """SEED_HI through the coupled kernel, at the tolerance of test_coupled_steps_match_the_twin (2e-4 (1 + |x|))."""
    rng = np.random.default_rng(d)
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    A = (Q * np.linspace(1.0, 20.0, d)) @ Q.T
    A32 = (0.5 * (A + A.T)).astype(np.float32)
    A32 = np.triu(A32) + np.triu(A32, 1).T
    b = rng.standard_normal(d).astype(np.float32)
    x0 = rng.standard_normal((chains, d)).astype(np.float32)
    lc = hip.LangevinChains(chains, d)
    try:
        lc.set_coupling(A32, b)
        lc.set_state(x0)
        traj = lc.step(12, 0.01, 1.0, 0.7, SEED, step0=5, chain0=3, trajectory=True)
        want, wtraj = ora.langevin_coupled_f32(x0, A32, b, 12, 0.01, 1.0, 0.7, SEED, step0=5, chain0=3, trajectory=True)
        got = lc.get_state()
        assert np.all(np.abs(got - want) <= 2e-4 * (1.0 + np.abs(want))), float(np.max(np.abs(got - want)))
        assert np.all(np.abs(traj - wtraj) <= 2e-4 * (1.0 + np.abs(wtraj)))
    finally:
        lc.close()


@pytest.mark.parametrize("d", [10, 65])
def test_k3_mixture(hip, d):
    """SEED_HI through both mixture kernels (one lane per chain up to dim 64, one workgroup above), at the tolerances of
    test_mixture_steps_match_the_twin: 2e-4 (1 + |x|) up to dim 64, 1e-3 (1 + |x|) above."""
    mix = _load("mixture_twin")
    K, chains = 3, 5
    rng = np.random.default_rng(1000 * d + K)
    base = rng.standard_normal(d)
    c = base[None, :] + (1.5 / np.sqrt(d)) * rng.standard_normal((K, d))
    w = rng.uniform(0.2, 2.0, K)
    x0 = (c[np.arange(chains) % K] + (0.5 / np.sqrt(d)) * rng.standard_normal((chains, d))).astype(np.float32)
    sigma = np.linspace(0.7, 1.4, K)
    lc = hip.LangevinChains(chains, d)
    try:
        lc.set_mixture(c, w, sigma, 1e-10)
        lc.set_state(x0)
        traj = lc.step(16, 0.01, 1.0, 0.3, SEED, step0=4, chain0=2, trajectory=True)
        got = lc.get_state()
        want, wtraj = mix.mixture_f32(x0, c, w, sigma, 1e-10, 16, 0.01, 1.0, 0.3, SEED, step0=4, chain0=2, trajectory=True)
        tol = 2e-4 if d <= 64 else 1e-3
        assert np.all(np.isfinite(got))
        assert np.all(np.abs(got - want) <= tol * (1.0 + np.abs(want))), float(np.max(np.abs(got - want)))
        assert np.all(np.abs(traj - wtraj) <= tol * (1.0 + np.abs(wtraj)))
    finally:
        lc.close()


# =================================================================================================== limits, from both sides

def _refused(hip, ctx, rc, text):
    assert rc == hip.TSU_E_INVALID, rc
    msg = ctx.lib.tsu_last_error(ctx.h).decode()
    assert text in msg, msg


def test_limits_of_the_lattice_entry_points(hip):
    """K1, K7, K8 sweeps: sweep0 + n = 2^31 + 1 and replica = 2^24 are refused by the C entry point (called below the wrapper's own
    check), nothing is launched, the spins stay; the wrappers raise ValueError for values outside the C types."""
    from ctypes import c_int8, c_uint32, c_uint64
    ctx = hip.Context.default()
    lib = ctx.lib
    rows, cols = 30, 48
    lat = hip.Lattice(rows, cols, True)
    l3 = hip.Lattice3D(4, 6, 8, True)
    try:
        lat.randomize(3)
        lat.set_model(1.0, 0.0, T_C)
        jr, jd, h = _gauss2d(rows, cols, True, 1)
        lat.set_disorder(jr, jd, h)
        l3.randomize(3)
        l3.set_disorder(*_gauss3d((4, 6, 8), True, 2))
        s2, s3 = lat.get_spins(), l3.get_spins()
        counts = (lat.launch_count(), lat.disorder_launch_count(), lat.cluster_launch_count(), l3.launch_count(), l3.cluster_launch_count())
        over, big = fe.LATTICE_LIMIT - 4, fe.REPLICA_LIMIT
        out = np.zeros((2, rows, cols), np.int8)
        outp = out.ctypes.data_as(hip._i8p)
        hs = (hip._vp * 1)(lat.h)
        one64, zero32 = (c_uint64 * 1)(1), (c_uint32 * 1)(0)
        for call, text in [
            (lambda: lib.tsu_ising2d_sweep(lat.h, 5, 1, over, 0), "sweep counter overflow"),
            (lambda: lib.tsu_ising2d_sweep(lat.h, 1, 1, 0, big), "2^24"),
            (lambda: lib.tsu_ising2d_sweep_part(lat.h, 1, 1, 0, big, hip.PART_ALL), "2^24"),
            (lambda: lib.tsu_ising2d_sample(lat.h, 1, 2, 2, 1, over, 0, outp), "sweep counter overflow"),
            (lambda: lib.tsu_ising2d_sample(lat.h, 1, 2, 2, 1, 0, big, outp), "2^24"),
            (lambda: lib.tsu_ising2d_sweep_batch(hs, 1, 5, one64, (c_uint32 * 1)(over), zero32), "sweep counter overflow"),
            (lambda: lib.tsu_ising2d_sweep_batch(hs, 1, 1, one64, zero32, (c_uint32 * 1)(big)), "2^24"),
            (lambda: lib.tsu_ising2d_randomize(lat.h, 1, big), "2^24"),
            (lambda: lib.tsu_ising2d_disorder_sweep(lat.h, 1.0, 5, 1, over, 0), "sweep counter overflow"),
            (lambda: lib.tsu_ising2d_disorder_sweep(lat.h, 1.0, 1, 1, 0, big), "2^24"),
        ]:
            _refused(hip, ctx, call(), text)
        for call, text in [
            (lambda: lib.tsu_ising3d_sweep(l3.h, 1.0, 5, 1, over, 0), "sweep counter overflow"),
            (lambda: lib.tsu_ising3d_sweep(l3.h, 1.0, 1, 1, 0, big), "2^24"),
            (lambda: lib.tsu_ising3d_randomize(l3.h, 1, big), "2^24"),
        ]:
            _refused(hip, ctx, call(), text)
        assert counts == (lat.launch_count(), lat.disorder_launch_count(), lat.cluster_launch_count(), l3.launch_count(),
                          l3.cluster_launch_count())
        _same(lat.get_spins(), s2, "2-D spins after the refused calls")
        _same(l3.get_spins(), s3, "3-D spins after the refused calls")
        # the wrappers: nothing wraps silently on its way into a C type
        for call in (lambda: lat.sweep(1, 1, 2 ** 32), lambda: lat.sweep(1, 1, -1), lambda: lat.sweep(1, 2 ** 64, 0), lambda: lat.sweep(1, -1, 0),
                     lambda: lat.sweep(1, 1, 0, 2 ** 24), lambda: lat.sweep(1, 1, 0, 2 ** 32 + 1), lambda: lat.randomize(1, 2 ** 24),
                     lambda: lat.sample(0, 1, 1, 1, 2 ** 32), lambda: lat.disorder_sweep(1.0, 1, 1, 2 ** 32 + 5),
                     lambda: lat.sweep(5, 1, over), lambda: lat.disorder_sweep(1.0, 5, 1, over), lambda: l3.sweep(1.0, 5, 1, over),
                     lambda: l3.sweep(1.0, 1, 1, 0, 2 ** 24), lambda: l3.randomize(2 ** 64),
                     lambda: hip.sweep_batch([lat], 1, [1], [2 ** 32], [0]), lambda: hip.sweep_batch([lat], 1, [1], [0], [2 ** 24]),
                     lambda: hip.sweep_batch([lat], 1, [2 ** 64], [0], [0])):
            with pytest.raises(ValueError):
                call()
        assert counts[0] == lat.launch_count() and counts[3] == l3.launch_count()
        _same(lat.get_spins(), s2, "2-D spins after the refused wrapper calls")
        # one sweep below the limit still runs (tests above run calls that end exactly at it)
        lat.sweep(4, 1, over)
        assert lat.launch_count() == counts[0] + 1
    finally:
        lat.close()
        l3.close()


def test_limits_of_the_cluster_steps(hip, monkeypatch):
    from ctypes import c_double, c_uint32, c_uint64
    ctx = hip.Context.default()
    lib = ctx.lib
    lat = hip.Lattice(37, 53, False)
    l3 = hip.Lattice3D(4, 6, 8, False)
    try:
        lat.randomize(3)
        l3.randomize(3)
        l3.set_disorder(*_gauss3d((4, 6, 8), False, 2, field=False))  # (zero field: both kinds of step take it)
        s2, s3 = lat.get_spins(), l3.get_spins()
        over, big = fe.COUNTER_LIMIT - 3, fe.REPLICA_LIMIT
        h2, h3 = (hip._vp * 1)(lat.h), (hip._vp * 1)(l3.h)
        one, one64, zero32 = (c_double * 1)(1.0), (c_uint64 * 1)(1), (c_uint32 * 1)(0)
        for call, text in [
            (lambda: lib.tsu_ising2d_cluster_sweep(lat.h, 1.0, 2.0, 4, 1, over, 0), "step counter overflow"),
            (lambda: lib.tsu_ising2d_cluster_sweep(lat.h, 1.0, 2.0, 1, 1, 0, big), "2^24"),
            (lambda: lib.tsu_ising2d_cluster_sweep_batch(h2, 1, 4, one, one, one64, (c_uint32 * 1)(over), zero32), "step counter overflow"),
            (lambda: lib.tsu_ising2d_cluster_sweep_batch(h2, 1, 1, one, one, one64, zero32, (c_uint32 * 1)(big)), "2^24"),
            (lambda: lib.tsu_ising3d_cluster_sweep(l3.h, 2.0, 4, 1, over, 0), "step counter overflow"),
            (lambda: lib.tsu_ising3d_cluster_sweep(l3.h, 2.0, 1, 1, 0, big), "2^24"),
            (lambda: lib.tsu_ising3d_cluster_sweep_field(l3.h, 2.0, 4, 1, over, 0), "step counter overflow"),
            (lambda: lib.tsu_ising3d_cluster_sweep_field(l3.h, 2.0, 1, 1, 0, big), "2^24"),
            (lambda: lib.tsu_ising3d_cluster_sweep_batch(h3, 1, 4, one, one64, (c_uint32 * 1)(over), zero32), "step counter overflow"),
            (lambda: lib.tsu_ising3d_cluster_sweep_batch(h3, 1, 1, one, one64, zero32, (c_uint32 * 1)(big)), "2^24"),
            (lambda: lib.tsu_ising3d_cluster_sweep_field_batch(h3, 1, 1, one, one64, zero32, (c_uint32 * 1)(big)), "2^24"),
        ]:
            _refused(hip, ctx, call(), text)
        for call in (lambda: lat.cluster_sweep(1.0, 2.0, 1, 1, 2 ** 32), lambda: lat.cluster_sweep(1.0, 2.0, 1, 1, 0, 2 ** 24),
                     lambda: lat.cluster_sweep(1.0, 2.0, 4, 1, over), lambda: l3.cluster_sweep(2.0, 1, 2 ** 64),
                     lambda: l3.cluster_sweep_field(2.0, 1, 1, 2 ** 32), lambda: l3.cluster_sweep(2.0, 1, 1, 0, 2 ** 24),
                     lambda: hip.cluster_sweep_batch([lat], 1, [1.0], [2.0], [1], [2 ** 32], [0]),
                     lambda: hip.cluster_sweep_batch_3d([l3], 1, [2.0], [1], [0], [2 ** 24])):
            with pytest.raises(ValueError):
                call()
        assert lat.cluster_launch_count() == 0 and l3.cluster_launch_count() == 0
        _same(lat.get_spins(), s2, "2-D spins")
        _same(l3.get_spins(), s3, "3-D spins")
        lat.cluster_sweep(1.0, 2.0, 3, 1, over)
        l3.cluster_sweep_field(2.0, 3, 1, over)
        assert lat.cluster_launch_count() == 1 and l3.cluster_launch_count() == 1
    finally:
        lat.close()
        l3.close()


def test_limits_of_the_dense_and_sparse_entry_points(hip):
    """tsu_dense_sweep / _sample / _anneal / _sweep_replicas and tsu_sparse_sweep / _sample: a sweep counter that would pass 2^32 is
    refused instead of wrapping to replay the stream of sweep 0; so is a replica id of 2^24."""
    from ctypes import c_double, c_uint32, c_uint64
    ctx = hip.Context.default()
    lib = ctx.lib
    n = 2304
    J, b, st = _dense_system(n, False, 1)
    d = hip.DenseSystem(J, b, hip.DTYPE_F32)
    A, bias, offsets, order, _, _ = _graph("chain", 40008)
    g = hip.SparseSystem(A.indptr, A.indices, A.data, bias, offsets, order)
    try:
        d.set_state(st)
        gs = np.random.default_rng(2).integers(0, 2, size=40008).astype(np.int8)
        g.set_state(gs)
        over, big = fe.COUNTER_LIMIT - 3, fe.REPLICA_LIMIT
        states = np.stack([st, st]).copy()
        sp = states.ctypes.data_as(hip._i8p)
        out = np.zeros((4, 40008), np.int8)
        outp = out.ctypes.data_as(hip._i8p)
        temps = (c_double * 4)(1.0, 1.0, 1.0, 1.0)
        for call, text in [
            (lambda: lib.tsu_dense_sweep(d.h, 1.0, 4, None, 1, over, 0, None), "dense_sweep: sweep counter overflow"),
            (lambda: lib.tsu_dense_sweep(d.h, 1.0, 1, None, 1, 0, big, None), "2^24"),
            (lambda: lib.tsu_dense_sample(d.h, 1.0, 2, 1, 2, None, 1, over, 0, None, outp), "dense_sample: sweep counter overflow"),
            (lambda: lib.tsu_dense_sample(d.h, 1.0, 0, 1, 1, None, 1, 0, big, None, outp), "2^24"),
            (lambda: lib.tsu_dense_anneal(d.h, temps, 4, None, 1, over, 0, None, outp), "dense_sample: sweep counter overflow"),
            (lambda: lib.tsu_dense_anneal(d.h, temps, 1, None, 1, 0, big, None, outp), "2^24"),
            (lambda: lib.tsu_dense_sweep_replicas(d.h, 2, temps, 4, sp, (c_uint64 * 2)(1, 2), (c_uint32 * 2)(0, over), (c_uint32 * 2)(0, 1), None),
             "dense_sweep_replicas: sweep counter overflow"),
            (lambda: lib.tsu_dense_sweep_replicas(d.h, 2, temps, 1, sp, (c_uint64 * 2)(1, 2), (c_uint32 * 2)(0, 0), (c_uint32 * 2)(0, big), None), "2^24"),
            (lambda: lib.tsu_sparse_sweep(g.h, 1.0, 4, 1, over, 0), "sparse_sweep: sweep counter overflow"),
            (lambda: lib.tsu_sparse_sweep(g.h, 1.0, 1, 1, 0, big), "2^24"),
            (lambda: lib.tsu_sparse_sample(g.h, 1.0, 2, 1, 2, 1, over, 0, outp), "sparse_sample: sweep counter overflow"),
            (lambda: lib.tsu_sparse_sample(g.h, 1.0, 0, 1, 1, 1, 0, big, outp), "2^24"),
        ]:
            _refused(hip, ctx, call(), text)
        for call in (lambda: d.sweep(1.0, 1, seed=1, sweep0=2 ** 32), lambda: d.sweep(1.0, 1, seed=2 ** 64), lambda: d.sweep(1.0, 1, replica=2 ** 24),
                     lambda: d.sweep(1.0, 4, seed=1, sweep0=over), lambda: d.sample(1.0, 0, 1, 1, sweep0=-1), lambda: d.anneal([1.0], sweep0=2 ** 32),
                     lambda: d.sweep_replicas(states, [1.0, 1.0], 1, [1, 2], [0, 2 ** 32]),
                     lambda: d.sweep_replicas(states, [1.0, 1.0], 1, [1, 2 ** 64], [0, 0]),
                     lambda: d.sweep_replicas(states, [1.0, 1.0], 1, [1, 2], [0, 0], replicas=[0, 2 ** 24]),
                     lambda: g.sweep(1.0, 1, seed=1, sweep0=2 ** 32), lambda: g.sweep(1.0, 4, seed=1, sweep0=over),
                     lambda: g.sweep(1.0, 1, seed=1, replica=2 ** 24), lambda: g.sample(1.0, 0, 1, 1, seed=2 ** 64)):
            with pytest.raises(ValueError):
                call()
        assert d.launch_counts() == (0, 0)
        _same(d.get_state(), st, "dense state")
        _same(g.get_state(), gs, "sparse state")
        _same(states, np.stack([st, st]), "replica states")
    finally:
        d.close()
        g.close()


# =================================================================================================== strip renumbering of k1_resident

def _resident_pair(hip, rows, cols, periodic, k):
    res, gen = hip.Lattice(rows, cols, periodic), hip.Lattice(rows, cols, periodic)
    res.set_kernel(hip.KERNEL_AUTO if periodic else hip.KERNEL_TILED, k)
    gen.set_kernel(hip.KERNEL_GENERIC, 0)
    table = TABLE()
    for lat in (res, gen):
        lat.randomize(SEED, REP)
        lat.set_thresholds(table)
    return res, gen


def _compare(res, gen, what):
    _same(res.get_spins(), gen.get_spins(), what)
    assert res.observables() == gen.observables(), what


@pytest.mark.parametrize("rows,cols,periodic", [(1024, 1024, True), (1000, 1000, True), (1000, 1000, False)])
def test_strip_numbering_crosses_two_restarts(hip, rows, cols, periodic):
    """One sweep per generation, calls of 1000 sweeps (one tile-resident launch each) until the numbering has restarted twice: about
    33 000 sweeps.  The twin handle runs the generic kernel (one thread per site, no tiles, no strips), which test_k1_routes pins to the
    oracle.  Compared before and after every call that restarts, and at the end; a restart comes exactly when
    generation + 1000 + 2 >= 16383, that is never earlier than one launch (1024 generations) before the limit."""
    call = 1000
    res, gen = _resident_pair(hip, rows, cols, periodic, 1)
    try:
        done, restarted = 0, 0
        assert res.strip_numbering() == (0, 0)
        while restarted < 2:
            g, r = res.strip_numbering()
            due = done > 0 and g + call + 2 >= GEN_LIMIT
            if due:
                assert g >= GEN_LIMIT - 2 - 1024
                _compare(res, gen, f"before the restart at sweep {done}")
            n0 = res.launch_count()
            res.sweep(call, SEED, done, REP)
            gen.sweep(call, SEED, done, REP)
            assert res.launch_count() - n0 == 1, "tile-resident: one launch per call"
            done += call
            if due:
                assert res.strip_numbering() == (call, r + 1), f"a restart was due at generation {g}"
                restarted += 1
                _compare(res, gen, f"after the restart at sweep {done}")
            else:
                assert res.strip_numbering() == (g + call, r if done > call else 1), f"no restart was due at generation {g}"
            assert done < 40 * GEN_LIMIT
        res.sweep(19, SEED, done, REP)
        gen.sweep(19, SEED, done, REP)
        _compare(res, gen, "at the end")
        assert gen.strip_numbering() == (0, 0)
    finally:
        res.close()
        gen.close()


def test_strip_numbering_of_nibble_planes(hip):
    """The same through the nibble planes' numbering (bits 32 .. 45 of an element), forced on 1024 x 1024 in a child process."""
    out = _child({"mode": "renumber", "rows": 1024, "cols": 1024, "periodic": 1, "seed": SEED, "replica": REP, "call": 1000, "restarts": 2},
                 {"TSU_TILE_VARIANT": "8"})
    assert "ok renumber 1024x1024" in out


def test_strip_layout_switches_on_a_live_handle(hip):
    """One 1024 x 1024 handle alternates one and two sweeps per generation between calls: every switch is another strip layout, the
    numbering restarts over a cleared buffer (one restart per switch), and the spins stay the generic twin's.  Calls of 9 sweeps are 9
    generations in the first layout and 5 in the second; calls of 5 sweeps in the first layout make the switch come after EQUAL
    numbers of generations, where a stale element of the old layout would carry exactly the numbers the new one asks for.  A reader
    takes such an element only if it looks before its neighbour has published, which is likeliest in a launch's first generations
    (the workgroups start apart): hence the two dozen switches of that kind, and two dozen more after calls of TWO generations (2
    sweeps at one per generation, 4 at two), whose stale elements carry the numbers 1 and 2."""
    res, gen = _resident_pair(hip, 1024, 1024, True, 1)
    try:
        done, restarts, prev_k = 0, 0, None
        for k, n in [(1, 9), (2, 9), (1, 9), (1, 5), (2, 9), (2, 9), (1, 9)] + 12 * [(1, 5), (2, 9)] + 24 * [(1, 2), (2, 4)]:
            res.set_kernel(hip.KERNEL_AUTO, k)
            n0 = res.launch_count()
            res.sweep(n, SEED, done, REP)
            gen.sweep(n, SEED, done, REP)
            assert res.launch_count() - n0 == 1
            done += n
            g, r = res.strip_numbering()
            gens = -(-n // k)
            if k != prev_k:
                restarts += 1
                assert (g, r) == (gens, restarts), f"k={k} n={n}: the switch did not restart the numbering"
            else:
                assert r == restarts and g > gens, f"k={k} n={n}: the numbering restarted without a switch"
            prev_k = k
            _compare(res, gen, f"after {done} sweeps (k = {k})")
    finally:
        res.close()
        gen.close()


def test_strip_numbering_of_two_periodic_slabs(hip):
    """Two 128 x 1024 slabs of a periodic 256 x 1024 lattice, tile-resident for every refresh period of 19 sweeps at one sweep per
    generation, driven until each slab's numbering has restarted once (863 periods); against the whole lattice on the generic
    kernel around the restart and at the end."""
    per, cols, ghost, k, nslab = 128, 1024, 40, 19, 2
    rows = per * nslab
    table = TABLE()
    full = ora.ising2d_randomize(rows, cols, SEED, REP)
    whole = hip.Lattice(rows, cols, True)
    slabs = [hip.Lattice(per, cols, True, total_rows=rows, row0=i * per, ghost=ghost) for i in range(nslab)]
    try:
        whole.set_kernel(hip.KERNEL_GENERIC, 0)
        whole.set_spins(full)
        whole.set_thresholds(table)
        for i, s in enumerate(slabs):
            s.set_kernel(hip.KERNEL_TILED, 1)
            s.set_spins(full[i * per:(i + 1) * per])
            s.set_thresholds(table)
        done, restarted = 0, False
        while not restarted:
            g, r = slabs[0].strip_numbering()
            due = done > 0 and g + k + 2 >= GEN_LIMIT
            owned = [s.get_spins() for s in slabs]
            if due:
                _same(np.concatenate(owned), whole.get_spins(), f"before the restart at sweep {done}")
            for i, s in enumerate(slabs):
                s.set_spins(owned[(i - 1) % nslab][-ghost:], row_first=-ghost)
                s.set_spins(owned[(i + 1) % nslab][:ghost], row_first=per)
            for s in slabs:
                n0 = s.launch_count()
                s.sweep(k, SEED, done, REP)
                assert s.launch_count() - n0 == 1, "a slab's refresh period is one tile-resident launch"
            whole.sweep(k, SEED, done, REP)
            done += k
            for s in slabs:
                assert s.strip_numbering() == ((k, r + 1) if due else (g + k, max(r, 1)))
            restarted = due
            assert done < 2 * GEN_LIMIT
        _same(np.concatenate([s.get_spins() for s in slabs]), whole.get_spins(), f"after the restart at sweep {done}")
    finally:
        whole.close()
        for s in slabs:
            s.close()

"""K10 (csrc/potts2d.hip, csrc/potts3d.hip) at its far ends, bit for bit against the NumPy twins (tests/helpers/potts_twin.py,
potts3d_twin.py): long axes and more than 524 288 sites (the second trip of the measuring kernels' grid-stride loop, Philox row and
octet words beyond 16 bits), the counters across 2^31 and 2^32 and the replica id 2^24 - 1 on both heat-bath routes, the limits of
tsu_potts*_run, the large and the degenerate cluster tiles in 3-D, one cluster across every seam and wrap, the low-half path of the
heat bath with its sites counted, two such sites in one octet, and the estimators of the temperature scans in exact rationals.
Seeds, replica ids and counter positions come from tests/helpers/far_end.py."""
import importlib.util
import math
import os
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fe = _load("far_end")
pt = _load("potts_twin")
p3 = _load("potts3d_twin")
OPEN, ALL = p3.OPEN, p3.ALL
FIELDS = {2: (0.0, 0.25), 3: (0.3, 0.0, -0.2), 5: (0.1, -0.3, 0.2, 0.0, 0.4), 8: fe.POTTS_FIELD8}
SMALL_SITES = 16384
T_NOMINAL_3D = 1.8  # times J: near the q = 3 transition of the cubic lattice


@pytest.fixture(scope="module")
def hip():
    from tsu import _hip
    return _hip


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in ("TSU_POTTS_SMALL", "TSU_SW3D_TILE", "TSU_SW_TILE"):
        monkeypatch.delenv(name, raising=False)


def _tc(q):
    return 1.0 / math.log(1.0 + math.sqrt(q))


def _twin(shape):
    return pt if len(shape) == 2 else p3


def _lattice(hip, shape, q, periodic):
    if len(shape) == 2:
        return hip.PottsLattice(shape[0], shape[1], q, periodic)
    return hip.PottsLattice3D(shape[0], shape[1], shape[2], q, periodic)


def _name(shape, kind):
    return ("k10_" if len(shape) == 2 else "k10_3d_") + kind


def _sid(shape, periodic):
    per = (periodic,) * len(shape) if isinstance(periodic, bool) else periodic
    return "x".join(map(str, shape)) + "-" + "".join("p" if x else "o" for x in per)


def _t_nominal(shape, q):
    return _tc(q) if len(shape) == 2 else T_NOMINAL_3D


def _start(shape, q, rng_seed=7):
    return np.random.default_rng(rng_seed).integers(0, q, size=shape).astype(np.int8)


def _set_tile(monkeypatch, shape, tile):
    """tile: None (the native route), an edge (2-D) or 'tz x tr x tc' (3-D)."""
    name = "TSU_SW_TILE" if len(shape) == 2 else "TSU_SW3D_TILE"
    if tile is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, str(tile))


def _launches_per_step(shape, periodic, tile):
    """Of the tiled route (sw_host.h): the local and the resolve pass, and the merge pass where a tile face or a wrap has bonds."""
    if len(shape) == 2:
        dims, per = (1,) + tuple(shape), (False, bool(periodic), bool(periodic))
        t = (1, int(tile), int(tile))
    else:
        dims, per = tuple(shape), p3.axes(periodic)
        t = tuple(int(v) for v in str(tile).split("x"))
    nz, nr, nc = (-(-n // e) for n, e in zip(dims, t))
    D, R, C = dims
    lanes = (nc - 1 + per[2]) * D * R + (nr - 1 + per[1]) * D * C + (nz - 1 + per[0]) * R * C
    return 3 if lanes > 0 else 2


def _check_measure(lat, s, q, periodic):
    n_eq, N = lat.measure()
    w_eq, w_N = _twin(s.shape).measure(s, q, periodic)
    assert n_eq == w_eq and N.tolist() == w_N.tolist(), (n_eq, w_eq, N.tolist(), w_N.tolist())


def _same(got, want, what):
    assert got.shape == want.shape and (got == want).all(), f"{what}: differs at {np.argwhere(got != want)[:5].tolist()}"


def _cluster_call(lat, twin, state, q, periodic, J, T, n, seed, step0, replica, what):
    """n cluster steps on the device and in the twin, compared; returns the new state."""
    want = twin.cluster_sweep(state, q, periodic, J, T, n, seed, step0, replica)
    lat.cluster_sweep(T, n, seed, step0, replica)
    _same(lat.get_spins(), want, what)  # get_spins raises if a union / find cap expired
    return want


# ---------------------------------------------------------------- long axes, more than 524 288 sites
# (shape, periodic, q, J, h and T of the heat bath, index of the Potts position, replica, J of the cluster steps, forced tile of the
# thin shapes).  70000 x 8 and 300 x 300 x 6: global rows to 69 999 and 89 999; 4 x 131088: whole octets (the 16-byte route) to
# o = 8192; 723 x 731: odd, open, the byte route; 34 x 128 x 128: the 16-byte route with both layer loads; 2 x 2 x 131090: the byte
# route to o = 8193 with double bonds on two axes (and natively the 16 x 32 x 32 tile: 4097 of them fill the chip).  Every one holds
# more than 2048 x 256 sites, so k10_measure / k10_3d_measure take a second trip of their grid-stride loop with a ragged end
LONG = [((70000, 8), True, 2, -1.0, FIELDS[2], 0.7, 0, fe.REPLICA_MAX, 1.0, "6"),
        ((4, 131088), True, 5, 1.0, None, 1.0, 1, fe.REPLICA_BYTES, 0.37, "6"),
        ((723, 731), False, 8, 0.37, FIELDS[8], 2.0, 2, fe.REPLICA_MAX, 2.5, None),
        ((34, 128, 128), ALL, 3, 1.0, FIELDS[3], 1.0, 0, fe.REPLICA_BYTES, 1.0, None),
        ((300, 300, 6), OPEN, 8, -1.0, None, 0.7, 1, fe.REPLICA_MAX, 0.37, "3x5x6"),
        ((2, 2, 131090), ALL, 2, 1.0, FIELDS[2], 2.0, 2, fe.REPLICA_BYTES, 2.5, "3x5x6")]


@pytest.mark.parametrize("case", LONG, ids=lambda c: _sid(c[0], c[1]))
def test_long_axes_and_a_second_trip_of_the_measure_loop(hip, monkeypatch, case):
    """From default_rng(7): n_eq and N_c of the start, 2 heat-bath sweeps at a Potts position of the far-end table with SEED_HI and
    a far-end replica id, n_eq and N_c again; then from the same start 2 cluster steps at end32(2) on the native tiles (0.8 of the
    nominal temperature, so that clusters cross tiles), and on the thin shapes 2 more across t = 2^31 under a forced small tile,
    where almost every site lies on a seam."""
    shape, periodic, q, J, h, T, pos, replica, Jc, tile = case
    twin = _twin(shape)
    assert int(np.prod(shape)) > 2048 * 256
    start = _start(shape, q)
    sweep0 = fe.potts_positions(2)[pos][1]
    lat = _lattice(hip, shape, q, periodic)
    try:
        assert lat.route() == _name(shape, "sweep") and lat.route(hip.POTTS_SWENDSEN_WANG) == _name(shape, "sw_tiles")
        lat.set_model(J, h)
        lat.set_spins(start)
        _check_measure(lat, start, q, periodic)
        n0 = lat.launch_count()
        lat.sweep(T, 2, fe.SEED_HI, sweep0, replica)
        assert lat.launch_count() - n0 == 4
        want = twin.sweep(start, q, periodic, J, h, T, 2, fe.SEED_HI, sweep0, replica)
        _same(lat.get_spins(), want, "heat bath")
        _check_measure(lat, want, q, periodic)
        # cluster steps
        Tc = 0.8 * _t_nominal(shape, q) * Jc
        lat.set_model(Jc)
        lat.set_spins(start)
        n0 = lat.launch_count()
        state = _cluster_call(lat, twin, start, q, periodic, Jc, Tc, 2, fe.SEED_HI, fe.end32(2), replica, "native tiles")
        assert lat.launch_count() - n0 == 2 * 3
        _check_measure(lat, state, q, periodic)
        if tile is not None:
            _set_tile(monkeypatch, shape, tile)
            assert lat.route(hip.POTTS_SWENDSEN_WANG) == _name(shape, "sw_tiles")
            n0 = lat.launch_count()
            state = _cluster_call(lat, twin, state, q, periodic, Jc, Tc, 2, fe.SEED_HI, fe.straddle32(3) + 1, replica, f"tile {tile}")
            assert lat.launch_count() - n0 == 2 * 3
            _check_measure(lat, state, q, periodic)
    finally:
        lat.close()


# ---------------------------------------------------------------- counters and replica ids on both heat-bath routes
SMALL_SHAPES = [((6, 10), True), ((33, 65), False), ((130, 128), True), ((4, 5, 6), (True, False, True)), ((18, 32, 32), ALL)]
SMALL_IDS = [_sid(*s) for s in SMALL_SHAPES]
# q, J, h, T: one model per Potts position (and per test below), every q and both signs of J
MODELS = [(2, -1.0, FIELDS[2], 0.7), (5, 1.0, FIELDS[5], 1.0), (8, 0.37, None, 2.0), (3, 1.0, FIELDS[3], 1.1)]


def _heat_bath_routes(shape):
    """(route, value of TSU_POTTS_SMALL or None) of the lattice."""
    if int(np.prod(shape)) <= SMALL_SITES:
        return ((_name(shape, "small"), None), (_name(shape, "sweep"), "0"))
    return ((_name(shape, "sweep"), None),)


def _on_route(monkeypatch, lat, route, switch):
    if switch is None:
        monkeypatch.delenv("TSU_POTTS_SMALL", raising=False)
    else:
        monkeypatch.setenv("TSU_POTTS_SMALL", switch)
    assert lat.route() == route


def _sweep_launches(route, n):
    return 1 if route.endswith("small") else 2 * n


@pytest.mark.parametrize("shape,periodic", SMALL_SHAPES, ids=SMALL_IDS)
def test_five_sweeps_from_every_potts_position(hip, monkeypatch, shape, periodic):
    """sweep0 = 2^30 - 3 (hs crosses 2^31), 2^31 - 3 (hs wraps through 2^32) and 2^32 - 3 (sweep0 + k wraps), one after the other on
    one handle, with SEED_HI and both far-end replica ids."""
    twin = _twin(shape)
    for route, switch in _heat_bath_routes(shape):
        for i, (name, sweep0) in enumerate(fe.potts_positions(5)):
            q, J, h, T = MODELS[i]
            replica = fe.REPLICAS[i % 2]
            state = _start(shape, q)
            lat = _lattice(hip, shape, q, periodic)
            try:
                _on_route(monkeypatch, lat, route, switch)
                lat.set_model(J, h)
                lat.set_spins(state)
                for s0 in (sweep0, (sweep0 + 5) % 2 ** 32):  # the second call starts past the crossing
                    n0 = lat.launch_count()
                    lat.sweep(T, 5, fe.SEED_HI, s0, replica)
                    assert lat.launch_count() - n0 == _sweep_launches(route, 5)
                    state = twin.sweep(state, q, periodic, J, h, T, 5, fe.SEED_HI, s0, replica)
                    _same(lat.get_spins(), state, f"{route} {name} sweep0={s0}")
                    _check_measure(lat, state, q, periodic)
            finally:
                lat.close()


@pytest.mark.parametrize("shape,periodic", SMALL_SHAPES, ids=SMALL_IDS)
def test_sweeps_s_and_s_plus_2_31_draw_the_same_streams(hip, monkeypatch, shape, periodic):
    """include/tsu_hip_potts.h: hs = 2 s + colour modulo 2^32, so sweeps s and s + 2^31 coincide.  The device at both against the
    twin at s, and the twin at both."""
    twin = _twin(shape)
    q, J, h, T = MODELS[3]
    start = _start(shape, q)
    for s in (7, 2 ** 31 - 2):  # the second: s + k crosses 2^31, s + 2^31 + k crosses 2^32
        want = twin.sweep(start, q, periodic, J, h, T, 3, fe.SEED_HI, s, fe.REPLICA_BYTES)
        assert (twin.sweep(start, q, periodic, J, h, T, 3, fe.SEED_HI, s + 2 ** 31, fe.REPLICA_BYTES) == want).all()
        assert (twin.sweep(start, q, periodic, J, h, T, 3, fe.SEED_HI, s + 2 ** 30, fe.REPLICA_BYTES) != want).any()
        for route, switch in _heat_bath_routes(shape):
            lat = _lattice(hip, shape, q, periodic)
            try:
                _on_route(monkeypatch, lat, route, switch)
                lat.set_model(J, h)
                for sweep0 in (s, s + 2 ** 31):
                    lat.set_spins(start)
                    lat.sweep(T, 3, fe.SEED_HI, sweep0, fe.REPLICA_BYTES)
                    _same(lat.get_spins(), want, f"{route} sweep0={sweep0}")
            finally:
                lat.close()


@pytest.mark.parametrize("shape,periodic", SMALL_SHAPES, ids=SMALL_IDS)
def test_the_largest_replica_id_and_one_past_it(hip, monkeypatch, shape, periodic):
    """Replica 2^24 - 1 and 2^24 - 2 against the twin (they differ: the top byte of the id reaches the counter word); 2^24 is
    refused by the wrapper and by the library, nothing launched, the state as it was."""
    twin = _twin(shape)
    q, J, h, T = MODELS[1]
    start = _start(shape, q)
    want = [twin.sweep(start, q, periodic, J, h, T, 2, fe.SEED_HI, fe.POTTS_HS_WRAP, r) for r in (fe.REPLICA_MAX, fe.REPLICA_MAX - 1)]
    assert (want[0] != want[1]).any()
    assert (want[0] != twin.sweep(start, q, periodic, J, h, T, 2, fe.SEED_HI, fe.POTTS_HS_WRAP, fe.REPLICA_MAX & 0xFFFF)).any()
    for route, switch in _heat_bath_routes(shape):
        lat = _lattice(hip, shape, q, periodic)
        try:
            _on_route(monkeypatch, lat, route, switch)
            lat.set_model(J, h)
            for r, w in zip((fe.REPLICA_MAX, fe.REPLICA_MAX - 1), want):
                lat.set_spins(start)
                lat.sweep(T, 2, fe.SEED_HI, fe.POTTS_HS_WRAP, r)
                _same(lat.get_spins(), w, f"{route} replica {r}")
            lat.set_spins(start)
            n0 = lat.launch_count()
            with pytest.raises(ValueError):
                lat.sweep(T, 2, fe.SEED_HI, fe.POTTS_HS_WRAP, fe.REPLICA_LIMIT)
            with pytest.raises(ValueError):
                lat.run(T, 2, 1, hip.POTTS_HEAT_BATH, fe.SEED_HI, 0, fe.REPLICA_LIMIT)
            sweep = lat.lib.tsu_potts2d_sweep if len(shape) == 2 else lat.lib.tsu_potts3d_sweep
            with pytest.raises(ValueError, match="2\\^24"):  # the library's own check, past the wrapper's
                lat.ctx.check(sweep(lat.h, T, 2, fe.SEED_HI, fe.POTTS_HS_WRAP, fe.REPLICA_LIMIT))
            assert lat.launch_count() == n0
            _same(lat.get_spins(), start, "after the refusals")
        finally:
            lat.close()
    # the cluster steps share the limit
    lat = _lattice(hip, shape, q, periodic)
    try:
        lat.set_spins(start)
        Tc = _t_nominal(shape, q)
        t0 = fe.straddle32(3) + 1  # t = 2^31 - 1 and 2^31
        state = _cluster_call(lat, twin, start, q, periodic, 1.0, Tc, 2, fe.SEED_HI, t0, fe.REPLICA_MAX, "replica 2^24 - 1")
        assert (state != twin.cluster_sweep(start, q, periodic, 1.0, Tc, 2, fe.SEED_HI, t0, fe.REPLICA_MAX - 1)).any()
        n0 = lat.launch_count()
        with pytest.raises(ValueError):
            lat.cluster_sweep(Tc, 2, fe.SEED_HI, 0, fe.REPLICA_LIMIT)
        with pytest.raises(ValueError):
            lat.run(Tc, 2, 1, hip.POTTS_SWENDSEN_WANG, fe.SEED_HI, 0, fe.REPLICA_LIMIT)
        assert lat.launch_count() == n0
        _same(lat.get_spins(), state, "after the refusals")
    finally:
        lat.close()


# ---------------------------------------------------------------- tsu_potts2d_run / tsu_potts3d_run at their limits
RUN_SHAPES = [((6, 10), True, 3), ((4, 5, 6), (True, False, True), 5)]


def _twin_rows(twin, start, q, periodic, update, counter0, n_meas, every, wrap):
    """The rows of a run from the twin alone: `update(state, n, counter)` n_meas times, a measurement after each."""
    rows, state = np.zeros((n_meas, 9), np.int64), start
    for k in range(n_meas):
        c = counter0 + k * every
        state = update(state, every, c % 2 ** 32 if wrap else c)
        n_eq, N = twin.measure(state, q, periodic)
        rows[k, 0], rows[k, 1:1 + q] = n_eq, N
    return rows, state


@pytest.mark.parametrize("shape,periodic,q", RUN_SHAPES, ids=["6x10", "4x5x6"])
def test_run_wraps_the_heat_bath_counter(hip, monkeypatch, shape, periodic, q):
    """counter0 = 2^32 - 5, 6 measurements 3 sweeps apart: the third call starts at sweep 1 of the next turn.  Rows and final state
    equal the twin's single calls with the counter taken modulo 2^32, on both routes."""
    twin = _twin(shape)
    J, h, T, seed, rep = -1.0, FIELDS[q], 0.9, fe.SEED_HI, fe.REPLICA_BYTES
    start = _start(shape, q)
    rows, end = _twin_rows(twin, start, q, periodic, lambda s, n, c: twin.sweep(s, q, periodic, J, h, T, n, seed, c, rep),
                           2 ** 32 - 5, 6, 3, True)
    for route, switch in _heat_bath_routes(shape):
        lat = _lattice(hip, shape, q, periodic)
        try:
            _on_route(monkeypatch, lat, route, switch)
            lat.set_model(J, h)
            lat.set_spins(start)
            n0 = lat.launch_count()
            lat.run(T, 6, 3, hip.POTTS_HEAT_BATH, seed, 2 ** 32 - 5, rep)
            assert lat.launch_count() - n0 == 6 * (_sweep_launches(route, 3) + 1)
            assert (lat.record() == rows).all(), route
            _same(lat.get_spins(), end, route)
        finally:
            lat.close()


@pytest.mark.parametrize("shape,periodic,q", RUN_SHAPES, ids=["6x10", "4x5x6"])
def test_run_ends_the_cluster_counter_at_its_limit(hip, monkeypatch, shape, periodic, q):
    """counter0 + n_meas every = 2^32 runs and equals the twin (one-workgroup route and forced tiles); one step more, by the counter
    or by the number of measurements, is refused: nothing launched, the state and the record as they were."""
    twin = _twin(shape)
    J, seed, rep = 1.0, fe.SEED_HI, fe.REPLICA_MAX
    T = _t_nominal(shape, q)
    start = _start(shape, q)
    c0 = fe.end32(18)
    rows, end = _twin_rows(twin, start, q, periodic, lambda s, n, c: twin.cluster_sweep(s, q, periodic, J, T, n, seed, c, rep),
                           c0, 6, 3, False)
    for tile in (None, "4" if len(shape) == 2 else "2x4x4"):
        _set_tile(monkeypatch, shape, tile)
        lat = _lattice(hip, shape, q, periodic)
        try:
            assert lat.route(hip.POTTS_SWENDSEN_WANG) == _name(shape, "sw_small" if tile is None else "sw_tiles")
            lat.set_spins(start)
            n0 = lat.launch_count()
            lat.run(T, 6, 3, hip.POTTS_SWENDSEN_WANG, seed, c0, rep)
            per_call = 1 if tile is None else 3 * _launches_per_step(shape, periodic, tile)
            assert lat.launch_count() - n0 == 6 * (per_call + 1)
            assert (lat.record() == rows).all(), tile
            _same(lat.get_spins(), end, f"tile {tile}")
            n0 = lat.launch_count()
            for bad in ((6, 3, c0 + 1), (7, 3, c0), (6, 4, c0), (19, 1, c0)):
                with pytest.raises(ValueError):
                    lat.run(T, bad[0], bad[1], hip.POTTS_SWENDSEN_WANG, seed, bad[2], rep)
            assert lat.launch_count() == n0
            assert (lat.record() == rows).all()
            _same(lat.get_spins(), end, "after the refusals")
            lat.run(T, 1, 1, hip.POTTS_SWENDSEN_WANG, seed, 2 ** 32 - 1, rep)  # the last step there is
            _same(lat.get_spins(), twin.cluster_sweep(end, q, periodic, J, T, 1, seed, 2 ** 32 - 1, rep), "t = 2^32 - 1")
        finally:
            lat.close()


# ---------------------------------------------------------------- large and degenerate tiles of k10_3d_sw_*
@pytest.mark.parametrize("q", [3, 8])
def test_large_tile_of_the_3d_cluster_steps(hip, monkeypatch, q):
    """16 x 32 x 32 tiles (80 KB of dynamic LDS, 1024 lanes: the default once they fill the chip), forced on 36 x 70 x 64 with a
    periodic column axis: 3 x 3 x 2 of them with ragged edges (K8's case in tests/test_cluster3d_gpu.py)."""
    shape, periodic = (36, 70, 64), (False, False, True)
    monkeypatch.setenv("TSU_SW3D_TILE", "16x32x32")
    start = _start(shape, q)
    lat = _lattice(hip, shape, q, periodic)
    try:
        assert lat.route(hip.POTTS_SWENDSEN_WANG) == "k10_3d_sw_tiles"
        lat.set_spins(start)
        n0 = lat.launch_count()
        T, t0 = 0.8 * T_NOMINAL_3D, fe.straddle32(3)
        state = _cluster_call(lat, p3, start, q, periodic, 1.0, T, 2, fe.SEED_HI, t0, fe.REPLICA_BYTES, "first call")
        state = _cluster_call(lat, p3, state, q, periodic, 1.0, T, 1, fe.SEED_HI, t0 + 2, fe.REPLICA_BYTES, "second call")
        assert lat.launch_count() - n0 == 9
        _check_measure(lat, state, q, periodic)
    finally:
        lat.close()


@pytest.mark.parametrize("shape,periodic", [((6, 10, 12), (True, False, True)), ((5, 7, 9), OPEN)], ids=["6x10x12-pop", "5x7x9-ooo"])
@pytest.mark.parametrize("tile", ["1x1x2", "2x64x8", "16x32x32"])
def test_degenerate_tiles_of_the_3d_cluster_steps(hip, monkeypatch, shape, periodic, tile):
    """A tile of two sites (every other bond on a seam, 64 lanes for 2 sites), a tile wider than the lattice on one axis and
    thinner on another, and one tile larger than the whole lattice (no seam; a merge pass only where an axis wraps): 3 steps at
    q = 3 and q = 8 from a random start, then 3 from the result at a lower temperature."""
    monkeypatch.setenv("TSU_SW3D_TILE", tile)
    for q, J in ((3, 1.0), (8, 0.37)):
        start = _start(shape, q)
        lat = _lattice(hip, shape, q, periodic)
        try:
            assert lat.route(hip.POTTS_SWENDSEN_WANG) == "k10_3d_sw_tiles"
            lat.set_model(J)
            lat.set_spins(start)
            n0 = lat.launch_count()
            T = T_NOMINAL_3D * J
            state = _cluster_call(lat, p3, start, q, periodic, J, T, 3, fe.SEED_HI, fe.end32(6), fe.REPLICA_MAX, f"q={q}")
            state = _cluster_call(lat, p3, state, q, periodic, J, 0.5 * T, 3, fe.SEED_HI, fe.end32(3), fe.REPLICA_MAX, f"q={q} cold")
            assert lat.launch_count() - n0 == 6 * _launches_per_step(shape, periodic, tile)
            _check_measure(lat, state, q, periodic)
        finally:
            lat.close()


# ---------------------------------------------------------------- one cluster across every seam and wrap
SPANNING = [((256, 512), True, None, 3), ((256, 512), True, "8", 8), ((24, 36, 68), ALL, None, 3), ((8, 16, 32), ALL, None, 8),
            ((8, 16, 32), ALL, "2x4x4", 2)]


@pytest.mark.parametrize("shape,periodic,tile,q", SPANNING,
                         ids=["x".join(map(str, s[0])) + "-" + (s[2] or "native") for s in SPANNING])
def test_one_cluster_spans_every_seam_and_wrap(hip, monkeypatch, shape, periodic, tile, q):
    """fill(c), then 1 + 3 steps at T = 0.01 J: -expm1(-100) rounds to 1, the threshold is 2^32 itself and every bond is active, so
    the lattice is one cluster whose root is site 0 (the twin's labels say so) and every step paints it with one colour: the
    hardest case for the agent-scope atomicMin merges and for the root chase, whose caps must not fire (get_spins would raise).
    Then 3 steps at the nominal temperature from that ordered state: large clusters, no longer total."""
    twin = _twin(shape)
    J, seed, rep = 2.5, fe.SEED_HI, fe.REPLICA_MAX
    T = 0.01 * J
    assert twin.threshold(J, T) == 2 ** 32
    _set_tile(monkeypatch, shape, tile)
    native = _name(shape, "sw_small" if int(np.prod(shape)) <= SMALL_SITES else "sw_tiles")
    lat = _lattice(hip, shape, q, periodic)
    try:
        assert lat.route(hip.POTTS_SWENDSEN_WANG) == (native if tile is None else _name(shape, "sw_tiles"))
        lat.set_model(J)
        lat.fill(q - 1)
        state = np.full(shape, q - 1, np.int8)
        _same(lat.get_spins(), state, "fill")
        n0 = lat.launch_count()
        for step0, n in ((fe.end32(4), 1), (fe.end32(3), 3)):
            last = twin.cluster_sweep(state, q, periodic, J, T, n - 1, seed, step0, rep)
            assert (twin.labels(last, periodic, J, T, seed, step0 + n - 1, rep) == 0).all()
            state = _cluster_call(lat, twin, state, q, periodic, J, T, n, seed, step0, rep, f"step0={step0}")
            assert (state == state.flat[0]).all()
        if native.endswith("sw_small") and tile is None:
            assert lat.launch_count() - n0 == 2
        else:
            assert lat.launch_count() - n0 == 4 * 3
        _check_measure(lat, state, q, periodic)
        Tn = _t_nominal(shape, q) * J
        after = _cluster_call(lat, twin, state, q, periodic, J, Tn, 3, seed, fe.straddle32(3), rep, "nominal T")
        assert (after != after.flat[0]).any()
        _check_measure(lat, after, q, periodic)
    finally:
        lat.close()


# ---------------------------------------------------------------- the low-half path of the heat bath
def _lo_case(twin, shape):
    """tests/test_potts_far_end_cpu.py's lo_case_counts: (start, final state, sites per octet position, octets with two)."""
    m = fe.POTTS_LO_MODEL
    start = _start(shape, m["q"])
    end, masks = twin.lo_trajectory(start, m["q"], True, m["J"], m["h"], m["T"], m["n_sweeps"], m["seed"], m["sweep0"], m["replica"])
    per_m, pairs = np.zeros(8, np.int64), 0
    for mask in masks:
        a, b = twin.lo_fold(mask)
        per_m += np.array(a)
        pairs += b
    return start, end, per_m.tolist(), pairs


@pytest.mark.parametrize("shape", [fe.POTTS_LO_SHAPE_3D, fe.POTTS_LO_SHAPE_2D], ids=["34x128x128", "1024x544"])
def test_sites_decided_by_the_low_half_at_every_octet_position(hip, shape):
    """q = 8, J = 1, h = FIELDS[8], T = 1, SEED_HI, sweep0 = 2^30 - 1 (hs crosses 2^31), replica 2^24 - 1, 2 sweeps from
    default_rng(7), whole octets (the 16-byte route).  Along the twin's trajectory the low half of u decides, per octet position
    m = 0 .. 7, (14, 19, 20, 9, 15, 17, 16, 15) sites on 34 x 128 x 128 (125 in all) and (16, 12, 17, 19, 7, 17, 22, 6) on
    1024 x 544 (116 in all), never two in one octet (tests/test_potts_far_end_cpu.py pins these).  At least 4 at every position is
    required of the inputs here, before the device is compared: a wrong lo16 half at any position changes a colour."""
    twin = _twin(shape)
    m = fe.POTTS_LO_MODEL
    start, want, per_m, pairs = _lo_case(twin, shape)
    print(f"\n{shape}: sites decided by the low half per octet position {per_m}, {sum(per_m)} in all, {pairs} octets with two")
    assert min(per_m) >= 4
    lat = _lattice(hip, shape, m["q"], True)
    try:
        assert lat.route() == _name(shape, "sweep")
        lat.set_model(m["J"], m["h"])
        lat.set_spins(start)
        n0 = lat.launch_count()
        lat.sweep(m["T"], m["n_sweeps"], m["seed"], m["sweep0"], m["replica"])
        assert lat.launch_count() - n0 == 2 * m["n_sweeps"]
        _same(lat.get_spins(), want, "low-half case")
        _check_measure(lat, want, m["q"], True)
    finally:
        lat.close()


@pytest.mark.parametrize("shape", [fe.POTTS_LO_PAIR_SHAPE_2D, fe.POTTS_LO_PAIR_SHAPE_3D], ids=["128x128", "8x16x128"])
@pytest.mark.parametrize("sweep,colour,rho,octet", fe.POTTS_LO_PAIRS)
def test_two_low_half_sites_in_one_octet_reuse_the_block(hip, monkeypatch, shape, sweep, colour, rho, octet):
    """J = 0, q = 8, h = FIELDS[8], T = 1, SEED_HI, replica 2^24 - 1: in half-sweep hs = 2 sweep + colour the octet (rho, octet)
    holds two sites that the low half decides (tools/potts_lo_pair_search.py), so the second one takes the lo16 block the first
    drew (d.have_lo).  One sweep from a random start on both heat-bath routes; 16384 sites, so k10_small / k10_3d_small take it."""
    twin = _twin(shape)
    m = fe.POTTS_LO_PAIR_MODEL
    start = _start(shape, m["q"])
    end, masks = twin.lo_trajectory(start, m["q"], True, m["J"], m["h"], m["T"], 1, m["seed"], sweep, m["replica"])
    assert twin.lo_octets(masks[colour])[rho, octet] >= 2
    assert (end == twin.sweep(start, m["q"], True, m["J"], m["h"], m["T"], 1, m["seed"], sweep, m["replica"])).all()
    for route, switch in _heat_bath_routes(shape):
        lat = _lattice(hip, shape, m["q"], True)
        try:
            _on_route(monkeypatch, lat, route, switch)
            lat.set_model(m["J"], m["h"])
            lat.set_spins(start)
            lat.sweep(m["T"], 1, m["seed"], sweep, m["replica"])
            _same(lat.get_spins(), end, route)
        finally:
            lat.close()


# ---------------------------------------------------------------- the estimators of the temperature scans
def _scan_reference(twin, shape, q, periodic, temperatures, n_equilibrate, n_measure, every, algorithm, seed):
    """What potts_temperature_scan(_3d) documents, from the twin's int64 rows in exact rational arithmetic: per temperature a fresh
    lattice from default_rng(seed), n_equilibrate updates from counter 0, then the measured updates from counter n_equilibrate
    (PottsModel2D / PottsModel3D count their sweeps and their cluster steps from 0).  e = -J n_eq / N, m = (q max N_c / N - 1) /
    (q - 1); energy = <e>, order_parameter = <m>, specific_heat = N var(e) / T^2, susceptibility = N var(m) / T with population
    variances, binder = 1 - <m^4> / (3 <m^2>^2)."""
    N = int(np.prod(shape))
    out = {k: [] for k in ("energy", "order_parameter", "specific_heat", "susceptibility", "binder")}
    for T in temperatures:
        state = np.random.default_rng(seed).integers(0, q, size=shape).astype(np.int8)
        if algorithm == "heat_bath":
            def update(s, n, c):
                return twin.sweep(s, q, periodic, 1.0, None, T, n, seed, c)
        else:
            def update(s, n, c):
                return twin.cluster_sweep(s, q, periodic, 1.0, T, n, seed, c)
        state = update(state, n_equilibrate, 0)
        rows, _ = _twin_rows(twin, state, q, periodic, update, n_equilibrate, n_measure, every, False)
        e = [Fraction(-int(r[0]), N) for r in rows]
        m = [(Fraction(q * int(max(r[1:1 + q])), N) - 1) / (q - 1) for r in rows]
        assert all(int(sum(r[1:1 + q])) == N for r in rows)

        def mean(x):
            return sum(x, Fraction(0)) / len(x)

        def var(x):
            mu = mean(x)
            return mean([(v - mu) ** 2 for v in x])
        Tq = Fraction(T)  # the float's exact value
        out["energy"].append(mean(e))
        out["order_parameter"].append(mean(m))
        out["specific_heat"].append(N * var(e) / Tq ** 2)
        out["susceptibility"].append(N * var(m) / Tq)
        out["binder"].append(1 - mean([v ** 4 for v in m]) / (3 * mean([v ** 2 for v in m]) ** 2))
    return out


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("algorithm", ["heat_bath", "swendsen_wang"])
def test_scan_estimators_in_exact_rationals(dim, algorithm):
    """potts_temperature_scan((6, 10), 3, [0.9, 1.4], 20, 30, 2, seed=3) and potts_temperature_scan_3d((4, 6, 6), ...): every value
    within relative 1e-12 of the rational result from the twin's rows.  float64 summation over 30 terms differs by a few 1e-15; a
    wrong power of T, factor N or variance convention differs by far more than 1e-12."""
    import tsu
    shape, twin, scan = ((6, 10), pt, tsu.potts_temperature_scan) if dim == 2 else ((4, 6, 6), p3, tsu.potts_temperature_scan_3d)
    temperatures = [0.9, 1.4]
    res = scan(shape, 3, temperatures, n_equilibrate=20, n_measure=30, measure_every=2, algorithm=algorithm, seed=3)
    ref = _scan_reference(twin, shape, 3, True, temperatures, 20, 30, 2, algorithm, 3)
    assert res["temperatures"].tolist() == temperatures
    for key, want in ref.items():
        assert res[key].shape == (2,)
        for i, w in enumerate(want):
            got = Fraction(float(res[key][i]))
            print(f"\n{dim}-D {algorithm} T={temperatures[i]} {key}: {float(res[key][i])!r}, exact {float(w)!r}")
            assert w != 0 and abs(got - w) <= Fraction(1, 10 ** 12) * abs(w), (key, i)
    for i in range(2):  # the estimators are not degenerate here: a variance of 0 would pass any power of T
        assert ref["specific_heat"][i] > 0 and ref["susceptibility"][i] > 0

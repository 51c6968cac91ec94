"""K7 replica cluster moves on the GPU (tsu_pt2d_set_cluster_moves / _cluster_move / _cluster_stats, csrc/ising2d_icm.hip): a pass
equals the NumPy twin (tests/helpers/icm_twin.py) bit for bit on both routes and for several tile edges, crafted states, the pass
counter, the statistics, whole runs against the ladder twin fed the device energies, exact conservation of E_a + E_b on dyadic
disorder, cluster_moves=0 changes nothing, launch counts, equilibrium against exact enumeration, the autocorrelation time of q against
the same ladder without the moves, and C-ABI errors."""
import importlib.util
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("icm_twin", os.path.join(HERE, "helpers", "icm_twin.py"))
twin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(twin)
dtwin = twin.disorder_twin

TS = [0.5, 1.0, 1.5, 2.5]
T_CUT = 1.2  # slots 0 and 1 take part


@pytest.fixture(scope="module")
def hip():
    from tsu import _hip
    return _hip


def _pm_j(rows, cols, periodic, seed):
    rng = np.random.default_rng(seed)
    jr = rng.choice([-1.0, 1.0], size=(rows, cols)).astype(np.float32)
    jd = rng.choice([-1.0, 1.0], size=(rows, cols)).astype(np.float32)
    if not periodic:
        jr[:, -1] = 0.0
        jd[-1, :] = 0.0
    return jr, jd, None


def _handle(hip, rows, cols, periodic, Ts, dis, seed, every=1, t_max=float("inf"), ladders=2):
    pt = hip.TemperingLattice(rows, cols, periodic, len(Ts), ladders)
    pt.set_disorder(*dis)
    pt.set_temperatures(Ts)
    if every is not None:
        pt.set_cluster_moves(every, t_max)
    pt.init(seed)
    return pt


def _pairs(rows, cols, R, seed):
    """Per slot a random a and b = a flipped at a density that runs from sparse clusters to a percolating one."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(R):
        a = rng.choice([-1, 1], size=(rows, cols)).astype(np.int8)
        dens = (0.3, 0.55, 0.45, 0.7)[i % 4]
        b = np.where(rng.random((rows, cols)) < dens, -a, a).astype(np.int8)
        out.append((a, b))
    return out


def _put(pt, pairs):
    for i, (a, b) in enumerate(pairs):
        pt.set_spins(0, i, a)
        pt.set_spins(1, i, b)


def _check_passes(pt, pairs, periodic, seed, Ts, t_max, n_passes, m0=0):
    """n_passes device passes against the twin: both walkers of every slot, then the statistics."""
    R = len(Ts)
    cur = [list(p) for p in pairs]
    clusters, flipped, passes = np.zeros(R, np.int64), np.zeros(R, np.int64), np.zeros(R, np.int64)
    for m in range(m0, m0 + n_passes):
        pt.cluster_move()
        for i in range(R):
            if Ts[i] <= t_max:
                st = {}
                cur[i] = list(twin.move(cur[i][0], cur[i][1], periodic, seed, m, i, st))
                clusters[i] += st["clusters"]
                flipped[i] += st["flipped"]
                passes[i] += 1
            for k in range(2):
                got = pt.get_spins(k, i)
                assert (got == cur[i][k]).all(), f"pass {m}, slot {i}, ladder {k}: {int((got != cur[i][k]).sum())} sites differ"
    return cur, passes, clusters, flipped


SMALL = [(6, 10, True), (37, 53, False), (1, 9, False), (9, 1, False), (4, 4, True), (128, 128, True)]
TILED = [(130, 200, False), (256, 256, True), (1024, 1024, True)]
CASES = [(s, None) for s in SMALL] + [(s, e) for s in SMALL + TILED for e in ("8", "22", "64")] + [(s, None) for s in TILED]


@pytest.mark.parametrize("shape,edge", CASES, ids=[f"{s[0]}x{s[1]}{'P' if s[2] else 'O'}-{e or 'default'}" for s, e in CASES])
def test_pass_equals_twin(hip, monkeypatch, shape, edge):
    rows, cols, periodic = shape
    if edge is None:
        monkeypatch.delenv("TSU_ICM_TILE", raising=False)
    else:
        monkeypatch.setenv("TSU_ICM_TILE", edge)
    seed = 100 + rows
    pt = _handle(hip, rows, cols, periodic, TS, _pm_j(rows, cols, periodic, 1), seed, 1, T_CUT)
    try:
        pairs = _pairs(rows, cols, len(TS), rows * 7 + cols)
        _put(pt, pairs)
        cur, passes, clusters, flipped = _check_passes(pt, pairs, periodic, seed, TS, T_CUT, 2)
        for i in (2, 3):  # above the cut-off: left alone
            assert (cur[i][0] == pairs[i][0]).all() and (cur[i][1] == pairs[i][1]).all()
        st = pt.cluster_stats()
        assert (st["passes"] == passes).all() and (st["clusters"] == clusters).all() and (st["flipped"] == flipped).all(), st
        assert st["pass_count"] == 2
        tiled = edge is not None or rows * cols > 16384
        assert st["launches"] == (6 if tiled else 2)
    finally:
        pt.close()


def _crafted(rows, cols):
    a = np.random.default_rng(3).choice([-1, 1], size=(rows, cols)).astype(np.int8)
    rr, cc = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    cross = (rr == 2) | (cc == 5)  # a full row and a full column: the cluster touches itself across both wraps
    return a, {"all_plus": np.zeros((rows, cols), bool), "all_minus": np.ones((rows, cols), bool),
               "checkerboard": ((rr + cc) & 1) == 0, "cross": cross}


@pytest.mark.parametrize("edge", [None, "8"])
def test_crafted_states(hip, monkeypatch, edge):
    rows, cols, periodic, seed = 8, 12, True, 41
    if edge is None:
        monkeypatch.delenv("TSU_ICM_TILE", raising=False)
    else:
        monkeypatch.setenv("TSU_ICM_TILE", edge)
    a, masks = _crafted(rows, cols)
    names = list(masks)
    Ts = [0.5, 0.6, 0.7, 0.8]
    pt = _handle(hip, rows, cols, periodic, Ts, _pm_j(rows, cols, periodic, 2), seed)
    try:
        pairs = [(a, np.where(masks[n], -a, a).astype(np.int8)) for n in names]
        _put(pt, pairs)
        moved_whole = set()
        for m in range(6):
            before = [(pt.get_spins(0, i), pt.get_spins(1, i)) for i in range(4)]
            pt.cluster_move()
            for i, n in enumerate(names):
                wa, wb = twin.move(before[i][0], before[i][1], periodic, seed, m, i)
                ga, gb = pt.get_spins(0, i), pt.get_spins(1, i)
                assert (ga == wa).all() and (gb == wb).all(), (n, m)
                if n == "all_plus":
                    assert (ga == before[i][0]).all() and (gb == before[i][1]).all()
                if n in ("all_minus", "cross"):  # one cluster: wholly flipped in both walkers, or untouched
                    fa, fb = ga != before[i][0], gb != before[i][1]
                    assert (fa == fb).all() and (not fa.any() or (fa == masks[n]).all())
                    moved_whole.add((n, bool(fa.any())))
        st = pt.cluster_stats()
        N = rows * cols
        assert (st["clusters"] == np.array([0, 6, 6 * (N // 2), 6])).all(), st
        assert st["flipped"][0] == 0 and st["flipped"][1] % N == 0 and st["flipped"][3] % (rows + cols - 1) == 0
        assert {("all_minus", True), ("all_minus", False)} <= moved_whole  # six coins: both outcomes seen for this seed
    finally:
        pt.close()


def test_serpentine_across_every_seam(hip, monkeypatch):
    """One site-wide snake through a 256 x 256 open lattice: every even row, joined alternately at the right and the left end.
    It crosses every tile seam and makes the longest union chains; one cluster, no budget error."""
    monkeypatch.delenv("TSU_ICM_TILE", raising=False)
    L, seed = 256, 17
    snake = np.zeros((L, L), bool)
    snake[0::2, :] = True
    snake[1::4, L - 1] = True
    snake[3::4, 0] = True
    a = np.random.default_rng(8).choice([-1, 1], size=(L, L)).astype(np.int8)
    b = np.where(snake, -a, a).astype(np.int8)
    assert len(np.unique(twin.roots(a, b, False)[snake])) == 1
    Ts = [0.5, 0.7]
    pt = _handle(hip, L, L, False, Ts, _pm_j(L, L, False, 2), seed)
    try:
        pairs = [(a, b), (b, a)]
        _put(pt, pairs)
        _check_passes(pt, pairs, False, seed, Ts, float("inf"), 4)
        st = pt.cluster_stats()  # would raise on an expired budget
        assert (st["clusters"] == 4).all() and (st["flipped"] % int(snake.sum()) == 0).all()
        assert st["flipped"].sum() > 0
    finally:
        pt.close()


def test_counter_advances(hip, monkeypatch):
    monkeypatch.delenv("TSU_ICM_TILE", raising=False)
    rows, cols, periodic, seed = 32, 48, True, 9
    pt = _handle(hip, rows, cols, periodic, TS, _pm_j(rows, cols, periodic, 2), seed)
    try:
        pairs = _pairs(rows, cols, len(TS), 5)
        _put(pt, pairs)
        first, *_ = _check_passes(pt, pairs, periodic, seed, TS, float("inf"), 1, m0=0)
        _put(pt, pairs)
        second, *_ = _check_passes(pt, pairs, periodic, seed, TS, float("inf"), 1, m0=1)
        assert any((first[i][0] != second[i][0]).any() for i in range(len(TS)))
        pt.init(seed)  # init zeroes the counter and the statistics; the setting survives
        assert pt.cluster_stats()["pass_count"] == 0 and pt.cluster_stats()["passes"].sum() == 0
        _put(pt, pairs)
        again, *_ = _check_passes(pt, pairs, periodic, seed, TS, float("inf"), 1, m0=0)
        assert all((first[i][k] == again[i][k]).all() for i in range(len(TS)) for k in range(2))
        pt.set_temperatures([0.5, 1.0, 1.5, 2.5])
        pt.set_cluster_moves(1, 0.7)
        pt.set_temperatures([0.9, 0.6, 0.5, 2.5])  # re-evaluated: slots 1 and 2 take part now
        pt.cluster_move()
        assert (pt.cluster_stats()["passes"] == np.array([1, 2, 2, 1])).all()
    finally:
        pt.close()


def _gauss(rows, cols, periodic, seed, field=True):
    rng = np.random.default_rng(seed)
    jr, jd = rng.normal(size=(rows, cols)).astype(np.float32), rng.normal(size=(rows, cols)).astype(np.float32)
    if not periodic:
        jr[:, -1] = 0.0
        jd[-1, :] = 0.0
    return jr, jd, (rng.normal(size=(rows, cols)).astype(np.float32) if field else None)


@pytest.mark.parametrize("rows,cols,periodic", [(16, 16, True), (37, 53, False)])
@pytest.mark.parametrize("every,t_max", [(1, float("inf")), (3, float("inf")), (1, 1.0)])
def test_run_parity_with_twin(hip, monkeypatch, rows, cols, periodic, every, t_max):
    monkeypatch.delenv("TSU_ICM_TILE", raising=False)
    Ts = list(np.linspace(0.3, 2.0, 6))  # t_max = 1.0 cuts the ladder in half
    dis = _gauss(rows, cols, periodic, 7 + rows)
    seed, R = 77, len(Ts)
    pt = _handle(hip, rows, cols, periodic, Ts, dis, seed, every, t_max)
    try:
        start = [[pt.get_spins(k, w) for w in range(R)] for k in range(2)]
        tw = twin.Ladders(start, periodic, dis, Ts, seed, every, t_max)
        for n_rounds, interval in ((4, 2), (3, 1)):
            pt.run(n_rounds, interval, swap=True, record=True)
            hist = pt.history()

            def energies(j, k):
                E = np.empty(R)
                E[hist["walker"][j, k]] = hist["E"][j, k]
                return E
            want = tw.run(n_rounds, interval, True, True, energies)
            assert (hist["walker"] == want["walker"]).all()
            assert (hist["M"] == want["M"]).all()
            assert (hist["q"] == want["q"]).all()
            st = pt.stats()
            assert (st["attempts"] == tw.attempts).all() and (st["accepts"] == tw.accepts).all()
            assert (st["walker_at_slot"] == tw.walker_at_slot).all()
            assert st["sweep_count"] == tw.sweeps and st["round_count"] == tw.rounds
        E, _ = pt.energies()
        for k in range(2):
            for i in range(R):
                w = tw.walker_at_slot[k, i]
                assert (pt.get_spins(k, i) == tw.spins[k][w]).all()
                assert E[k, w] == pytest.approx(dtwin.energy(tw.spins[k][w], periodic, *dis), rel=1e-12, abs=1e-9)
        # the recorded q row of the last round is the overlap of the spins as they stand
        q_now = [int((pt.get_spins(0, i).astype(np.int64) * pt.get_spins(1, i)).sum()) for i in range(R)]
        assert (hist["q"][-1] == np.array(q_now)).all()
        cs = pt.cluster_stats()
        assert cs["pass_count"] == tw.passes and (cs["passes"] == tw.slot_passes).all()
        assert (cs["clusters"] == tw.clusters).all() and (cs["flipped"] == tw.flipped).all()
        assert tw.flipped.sum() > 0 and tw.accepts.sum() > 0
        assert (cs["passes"][np.array(Ts) > t_max] == 0).all()
    finally:
        pt.close()


def test_split_runs_equal_one_run(hip, monkeypatch):
    from tsu.models.ising import LatticeTempering
    monkeypatch.delenv("TSU_ICM_TILE", raising=False)
    jr, jd, h = _gauss(24, 20, True, 5)
    Ts = np.linspace(0.5, 2.5, 6)
    kw = dict(couplings=(jr, jd), field=h, seed=9, ladders=2, cluster_moves=2, cluster_max_temperature=1.5)
    a, b = LatticeTempering((24, 20), Ts, **kw), LatticeTempering((24, 20), Ts, **kw)
    try:
        a.run(3, 5)
        ha = a.run(4, 5)
        hb = b.run(7, 5)
        for key in ("E", "M", "walker", "q"):
            assert np.array_equal(ha[key], hb[key][3:]), key
        for key in ("passes", "clusters", "flipped"):
            assert np.array_equal(a.cluster_stats[key], b.cluster_stats[key]), key
        assert (a.cluster_stats["passes"] == np.array([4, 4, 4, 0, 0, 0])).all()  # rounds 0, 2, 4, 6; T <= 1.5
        for k in range(2):
            for i in range(len(Ts)):
                assert (a.spins(i, k) == b.spins(i, k)).all()
        a.cluster_move()
        assert (a.cluster_stats["passes"] == np.array([5, 5, 5, 0, 0, 0])).all()
    finally:
        a._pt.close()
        b._pt.close()


@pytest.mark.parametrize("rows,cols,periodic,edge", [(12, 16, True, None), (12, 16, True, "8"), (140, 130, False, None)])
def test_energy_sum_conserved_exactly(hip, monkeypatch, rows, cols, periodic, edge):
    """Dyadic couplings and fields: the device's float64 energies are exact, and E_a + E_b is equal before and after a pass."""
    if edge is None:
        monkeypatch.delenv("TSU_ICM_TILE", raising=False)
    else:
        monkeypatch.setenv("TSU_ICM_TILE", edge)
    rng = np.random.default_rng(rows)
    jr = rng.choice([-1.0, 1.0, 0.5, -0.25], size=(rows, cols)).astype(np.float32)
    jd = rng.choice([-1.0, 1.0, 0.5, -0.25], size=(rows, cols)).astype(np.float32)
    if not periodic:
        jr[:, -1] = 0.0
        jd[-1, :] = 0.0
    h = (rng.integers(-8, 9, size=(rows, cols)) / 4.0).astype(np.float32)
    pt = _handle(hip, rows, cols, periodic, TS, (jr, jd, h), 3)
    try:
        pt.run(2, 3, swap=True, record=False)
        was = pt.stats()["walker_at_slot"]
        E0, _ = pt.energies()
        spins0 = [pt.get_spins(0, i) for i in range(len(TS))]
        pt.cluster_move()
        E1, _ = pt.energies()
        moved = 0
        for i in range(len(TS)):
            wa, wb = was[0, i], was[1, i]
            assert E0[0, wa] + E0[1, wb] == E1[0, wa] + E1[1, wb], i
            moved += int((pt.get_spins(0, i) != spins0[i]).sum())
        assert moved > 0
    finally:
        pt.close()


def test_switched_off_changes_nothing(hip):
    rows, cols, periodic, seed = 20, 24, True, 31
    dis = _gauss(rows, cols, periodic, 2)
    plain = _handle(hip, rows, cols, periodic, TS, dis, seed, every=None)
    off = _handle(hip, rows, cols, periodic, TS, dis, seed, every=0)
    onoff = _handle(hip, rows, cols, periodic, TS, dis, seed, every=2, t_max=1.0)
    try:
        onoff.set_cluster_moves(0, 1.0)
        hs = []
        for pt in (plain, off, onoff):
            pt.run(5, 3, swap=True, record=True)
            hs.append(pt.history())
        for pt, h in zip((off, onoff), hs[1:]):
            for key in ("E", "M", "walker", "q"):
                assert np.array_equal(h[key], hs[0][key]), key
            sa, sb = pt.stats(), plain.stats()
            for key in sa:
                assert np.array_equal(sa[key], sb[key]), key
            for k in range(2):
                for i in range(len(TS)):
                    assert (pt.get_spins(k, i) == plain.get_spins(k, i)).all()
            assert pt.launch_count() == plain.launch_count() == 2 * 3 * 5
            cs = pt.cluster_stats()
            assert cs["pass_count"] == 0 and cs["launches"] == 0
            assert not cs["passes"].any() and not cs["clusters"].any() and not cs["flipped"].any()
    finally:
        for pt in (plain, off, onoff):
            pt.close()


@pytest.mark.parametrize("edge,per_pass", [(None, 1), ("8", 3)])
@pytest.mark.parametrize("R", [3, 8])
def test_launches_per_pass(hip, monkeypatch, edge, per_pass, R):
    if edge is None:
        monkeypatch.delenv("TSU_ICM_TILE", raising=False)
    else:
        monkeypatch.setenv("TSU_ICM_TILE", edge)
    Ts = list(np.linspace(0.4, 2.0, R))
    pt = _handle(hip, 16, 16, True, Ts, _pm_j(16, 16, True, 1), 5)
    try:
        pt.cluster_move()
        pt.cluster_move()
        assert pt.cluster_stats()["launches"] == 2 * per_pass
        n0 = pt.launch_count()
        pt.run(4, 2, swap=True, record=False)  # the sweep launches are counted apart from the passes'
        assert pt.launch_count() - n0 == 2 * 2 * 4
        assert pt.cluster_stats()["launches"] == 6 * per_pass
    finally:
        pt.close()


def _exact(jr, jd, h, periodic, Ts):
    """<E>/N and <q^2> of two independent replicas by enumerating every state; <q^2> = sum_ij <s_i s_j>^2 / N^2 also in a field."""
    rows, cols = jr.shape
    N = rows * cols
    idx = np.arange(2 ** N, dtype=np.int64)
    S = np.empty((2 ** N, N), np.int8)
    for n in range(N):
        S[:, n] = 1 - 2 * ((idx >> n) & 1)
    E = np.zeros(2 ** N)
    for r in range(rows):
        for c in range(cols):
            n = r * cols + c
            if periodic or c + 1 < cols:
                E -= float(jr[r, c]) * (S[:, n] * S[:, r * cols + (c + 1) % cols])
            if periodic or r + 1 < rows:
                E -= float(jd[r, c]) * (S[:, n] * S[:, ((r + 1) % rows) * cols + c])
            if h is not None:
                E -= float(h[r, c]) * S[:, n]
    out = []
    for T in Ts:
        w = np.exp(-(E - E.min()) / T)
        w /= w.sum()
        C = np.zeros((N, N))
        for lo in range(0, 2 ** N, 1 << 16):
            Sb = S[lo:lo + (1 << 16)].astype(np.float64)
            C += Sb.T @ (Sb * w[lo:lo + (1 << 16), None])
        out.append((float(w @ E) / N, float((C ** 2).sum()) / N ** 2))
    return out


@pytest.mark.parametrize("rows,cols,periodic,field", [(4, 4, True, False), (4, 5, False, False), (4, 4, True, True)])
def test_equilibrium_against_exact_enumeration(hip, monkeypatch, rows, cols, periodic, field):
    """The ladder, run lengths, 20 batches and the 4 s.e. + 1e-4 rule of test_tempering_gpu, with a pass in every round: a move that
    is a valid-looking but biased map (wrong adjacency on the wrap, a coin read at a non-root) shows here."""
    from tsu.models.ising import LatticeTempering
    monkeypatch.delenv("TSU_ICM_TILE", raising=False)
    jr, jd, h = _gauss(rows, cols, periodic, 21, field=field)
    Ts = np.linspace(0.3, 2.0, 8)
    N = rows * cols
    pt = LatticeTempering((rows, cols), Ts, couplings=(jr, jd), field=h, periodic=periodic, seed=5, ladders=2, cluster_moves=1)
    try:
        pt.run(400, 5, record=False)
        hist = pt.run(8000, 5)
        nb = 20
        exact = _exact(jr, jd, h, periodic, Ts)
        for i, (e_ex, q2_ex) in enumerate(exact):
            e_b = (hist["E"][:, i] / N).reshape(nb, -1).mean(axis=1)
            q_b = ((hist["q"][:, i] / N) ** 2).reshape(nb, -1).mean(axis=1)
            for b, ex in ((e_b, e_ex), (q_b, q2_ex)):
                se = b.std(ddof=1) / math.sqrt(nb)
                print(f"T={Ts[i]:.3f} mean={b.mean():+.6f} exact={ex:+.6f} se={se:.2e}")
                assert abs(b.mean() - ex) < 4 * se + 1e-4, (i, Ts[i], b.mean(), ex, se)
        cs = pt.cluster_stats
        assert (cs["passes"] == 8400).all() and (cs["flipped"] > 0).all()
    finally:
        pt._pt.close()


def _tau_int(x, c=6.0):
    """integrated autocorrelation time with Sokal's automatic window (the rule of tests/test_cluster_gpu.py)"""
    x = np.asarray(x, float) - np.mean(x)
    n = len(x)
    f = np.fft.rfft(x, 2 * n)
    acf = np.fft.irfft(f * np.conj(f))[:n]
    acf /= acf[0]
    tau = 0.5
    for w in range(1, n):
        tau += acf[w]
        if w >= c * tau:
            break
    return tau


def test_cluster_moves_decorrelate_the_coldest_slot(hip, monkeypatch):
    """The measurement of tools/icm_time.py part (b) (profiles/icm_time.txt): 32^2 +-J (disorder seed 1), 16 temperatures
    0.2 ... 1.6, ladder seed 3, one sweep per round, 20000 rounds discarded and 200000 measured.  The yardstick is the same ladder
    with cluster_moves=0.  Measured: tau_int(q) at the coldest slot 73.2 rounds without and 0.8 with the moves, ratio 97; the
    bound is half the measured ratio (the factor 2 absorbs the scatter of a tau estimated from a run of a few hundred tau)."""
    from tsu.models.ising import LatticeTempering
    monkeypatch.delenv("TSU_ICM_TILE", raising=False)
    L, n_eq, n = 32, 20000, 200000
    Ts = np.linspace(0.2, 1.6, 16)
    jr, jd, _ = _pm_j(L, L, True, 1)
    tau, trips = {}, {}
    for cm in (0, 1):
        pt = LatticeTempering(L, Ts, couplings=(jr, jd), seed=3, ladders=2, cluster_moves=cm)
        try:
            pt.run(n_eq, 1, record=False)
            q = np.concatenate([pt.run(50000, 1)["q"][:, 0] for _ in range(n // 50000)]) / float(L * L)
            tau[cm], trips[cm] = _tau_int(q), pt.round_trips
        finally:
            pt._pt.close()
    print(f"\n32^2 +-J, T = 0.2: tau_int(q) {tau[0]:.1f} rounds without, {tau[1]:.1f} with cluster moves, ratio {tau[0] / tau[1]:.1f}; "
          f"round trips {trips[0]} / {trips[1]}")
    assert tau[0] >= 48.0 * tau[1], (tau, trips)


def test_tempering_scan_reports_flipped_fraction(hip):
    from tsu.models.ising import tempering_scan
    jr, jd, _ = _pm_j(16, 16, True, 4)
    Ts = [0.4, 0.8, 1.6, 3.2]
    kw = dict(n_equilibrate=20, n_measure=6, measure_every=4, seed=3, couplings=(jr, jd), replicas=2)
    out = tempering_scan(16, Ts, cluster_moves=1, cluster_max_temperature=1.0, **kw)
    f = out["cluster_flipped"]
    assert f.shape == (4,) and np.isnan(f[2:]).all() and ((f[:2] >= 0) & (f[:2] <= 1)).all()
    assert "cluster_flipped" not in tempering_scan(16, Ts, **kw)


def test_errors(hip):
    z = np.zeros((8, 8), np.float32)
    one = hip.TemperingLattice(8, 8, True, 4, 1)
    try:
        with pytest.raises(ValueError, match="two ladders"):
            one.set_cluster_moves(1, 1.0)
        one.set_cluster_moves(0, 1.0)  # off is what it already is
    finally:
        one.close()
    pt = hip.TemperingLattice(8, 8, True, 4, 2)
    try:
        with pytest.raises(ValueError, match="every"):
            pt.set_cluster_moves(-1, 1.0)
        for bad in (0.0, -1.0, float("nan")):
            with pytest.raises(ValueError, match="t_max"):
                pt.set_cluster_moves(1, bad)
        with pytest.raises(ValueError, match="set_cluster_moves"):
            pt.cluster_move()
        pt.set_cluster_moves(1, float("inf"))  # before the temperatures: evaluated when they come
        with pytest.raises(ValueError, match="set_temperatures"):
            pt.cluster_move()
        pt.set_disorder(z, z)
        pt.set_temperatures([0.5, 1.0, 2.0, 3.0])
        with pytest.raises(ValueError, match="init"):
            pt.cluster_move()
        pt.init(3)
        pt.cluster_move()
        assert (pt.cluster_stats()["passes"] == 1).all()
    finally:
        pt.close()

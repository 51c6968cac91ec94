"""K7 replica cluster moves on the host: invariants of the NumPy twin (tests/helpers/icm_twin.py) on random, crafted and
exhaustively enumerated states (E_a + E_b exact on dyadic disorder, q unchanged per site, a same-counter pass is an involution),
the twin's equilibrium against exact enumeration, validation before the device is touched, and the new C-ABI symbols (no GPU)."""
import ctypes
import importlib.util
import math
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_spec = importlib.util.spec_from_file_location("icm_twin", os.path.join(HERE, "helpers", "icm_twin.py"))
twin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(twin)
dtwin = twin.disorder_twin

ICM_SYMBOLS = ["tsu_pt2d_set_cluster_moves", "tsu_pt2d_cluster_move", "tsu_pt2d_cluster_stats"]


def _dyadic(rows, cols, periodic, rng, field=True):
    jr = rng.choice([-1.0, 1.0, 0.5, -0.25], size=(rows, cols)).astype(np.float32)
    jd = rng.choice([-1.0, 1.0, 0.5, -0.25], size=(rows, cols)).astype(np.float32)
    if not periodic:
        jr[:, -1] = 0.0
        jd[-1, :] = 0.0
    h = (rng.integers(-8, 9, size=(rows, cols)) / 4.0).astype(np.float32) if field else None
    return jr, jd, h


def _energy(s, periodic, jr, jd, h):
    """-sum J s s' - sum h s in float64, whatever the shape (a wrap onto the same neighbour twice counts both bonds)."""
    s = np.asarray(s, np.float64)
    e = 0.0
    if periodic:
        e -= float((jr * s * np.roll(s, -1, 1)).sum()) + float((jd * s * np.roll(s, -1, 0)).sum())
    else:
        e -= float((jr[:, :-1] * s[:, :-1] * s[:, 1:]).sum()) + float((jd[:-1] * s[:-1] * s[1:]).sum())
    if h is not None:
        e -= float((h * s).sum())
    return e


def _check_invariants(a, b, periodic, dis, seed, m, slot):
    st = {}
    a2, b2 = twin.move(a, b, periodic, seed, m, slot, st)
    assert (a2.astype(np.int64) * b2 == a.astype(np.int64) * b).all()  # q per site
    assert ((a2 != a) == (b2 != b)).all() and not ((a2 != a) & (a.astype(np.int64) * b > 0)).any()
    assert _energy(a, periodic, *dis) + _energy(b, periodic, *dis) == _energy(a2, periodic, *dis) + _energy(b2, periodic, *dis)
    a3, b3 = twin.move(a2, b2, periodic, seed, m, slot)
    assert (a3 == a).all() and (b3 == b).all()  # the same counters: an involution
    assert st["flipped"] == int((a2 != a).sum())
    return a2, b2, st


@pytest.mark.parametrize("rows,cols,periodic", [(3, 3, False), (4, 4, True), (6, 10, True), (37, 53, False), (33, 70, True),
                                                (1, 9, True), (9, 2, True), (1, 9, False), (9, 1, False)])
def test_invariants_on_random_states(rows, cols, periodic):
    rng = np.random.default_rng(rows * 100 + cols)
    dis = _dyadic(rows, cols, periodic, rng)
    moved = 0
    for trial in range(12):
        a = rng.choice([-1, 1], size=(rows, cols)).astype(np.int8)
        b = np.where(rng.random((rows, cols)) < rng.choice([0.2, 0.5, 0.7]), -a, a).astype(np.int8)
        _, _, st = _check_invariants(a, b, periodic, dis, int(rng.integers(0, 2 ** 40)), trial, trial % 5)
        moved += st["flipped"]
    assert moved > 0


def test_energy_module_agrees_with_disorder_twin():
    rng = np.random.default_rng(2)
    for rows, cols, periodic in ((6, 10, True), (5, 7, False)):
        dis = _dyadic(rows, cols, periodic, rng)
        s = rng.choice([-1, 1], size=(rows, cols)).astype(np.int8)
        assert _energy(s, periodic, *dis) == dtwin.energy(s, periodic, *dis)


def _states(n_sites, shape, which):
    bits = (np.asarray(which, np.int64)[:, None] >> np.arange(n_sites)) & 1
    return (1 - 2 * bits).astype(np.int8).reshape((-1,) + shape)


@pytest.mark.parametrize("rows,cols,periodic,fraction", [(2, 3, False, 1.0), (3, 2, True, 1.0), (3, 3, False, 0.1)])
def test_every_joint_state_of_tiny_lattices(rows, cols, periodic, fraction):
    """Every (a, b) of the 2 x 3 open and 3 x 2 periodic lattices (4096 pairs each; with two columns the wrap reaches the same
    neighbour twice), a random tenth of the 2^18 pairs of 3 x 3 open (the cap is for time only)."""
    N = rows * cols
    rng = np.random.default_rng(N)
    dis = _dyadic(rows, cols, periodic, rng)
    total = 4 ** N
    which = np.arange(total) if fraction == 1.0 else rng.choice(total, size=int(total * fraction), replace=False)
    A = _states(N, (rows, cols), which & (2 ** N - 1))
    B = _states(N, (rows, cols), which >> N)
    images = set()
    for j in range(len(which)):
        a2, b2, _ = _check_invariants(A[j], B[j], periodic, dis, 12345, 3, 1)
        images.add((a2.tobytes(), b2.tobytes()))
    assert len(images) == len(which)  # a bijection on what was enumerated


def test_crafted_states():
    rows, cols = 8, 12
    rng = np.random.default_rng(3)
    a = rng.choice([-1, 1], size=(rows, cols)).astype(np.int8)
    rr, cc = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    dis = _dyadic(rows, cols, True, rng)
    # all q = +1: nothing moves, no cluster
    a2, b2, st = _check_invariants(a, a.copy(), True, dis, 7, 0, 0)
    assert st == {"clusters": 0, "flipped": 0} and (a2 == a).all() and (b2 == a).all()
    # all q = -1: one cluster rooted at site 0; both walkers wholly flipped or untouched, both outcomes over a few counters
    seen = set()
    for m in range(12):
        a2, b2, st = _check_invariants(a, (-a).astype(np.int8), True, dis, 7, m, 2)
        assert st["clusters"] == 1 and st["flipped"] in (0, rows * cols)
        assert (twin.roots(a, -a, True) == 0).all()
        seen.add(st["flipped"])
    assert seen == {0, rows * cols}
    # checkerboard q: N / 2 single-site clusters, each its own root, about half of them flipped
    board = ((rr + cc) & 1) == 0
    b = np.where(board, -a, a).astype(np.int8)
    _, _, st = _check_invariants(a, b, True, dis, 7, 0, 1)
    rt = twin.roots(a, b, True)
    assert st["clusters"] == rows * cols // 2 and (rt[board] == (rr * cols + cc)[board]).all() and (rt[~board] == -1).all()
    assert 8 <= st["flipped"] <= 40
    # a full row and a full column: one cluster that touches itself across both wraps; on the open lattice still one
    cross = (rr == 2) | (cc == 5)
    b = np.where(cross, -a, a).astype(np.int8)
    for periodic in (True, False):
        d = _dyadic(rows, cols, periodic, rng)
        _, _, st = _check_invariants(a, b, periodic, d, 7, 1, 0)
        assert st["clusters"] == 1 and (twin.roots(a, b, periodic)[cross] == 5).all()
    # two segments of the top row that only the wrap joins
    seg = np.zeros((rows, cols), bool)
    seg[0, :3] = seg[0, -2:] = True
    b = np.where(seg, -a, a).astype(np.int8)
    assert len(np.unique(twin.roots(a, b, True)[seg])) == 1 and len(np.unique(twin.roots(a, b, False)[seg])) == 2
    # J = 0 on a bond does not cut a cluster: adjacency is the lattice's
    jr, jd, h = _dyadic(rows, cols, True, rng)
    jr[0, 0] = 0.0
    assert len(np.unique(twin.roots(a, b, True)[seg])) == 1
    _check_invariants(a, b, True, (jr, jd, h), 7, 0, 0)


def test_coin_is_flip_bit_of_the_root():
    """The coin restated from the contract: bit 31 of word c & 3 of Philox(c >> 2, r, m, 9 | slot << 8)."""
    rows, cols, seed, m, slot = 5, 11, (3 << 32) | 77, 6, 4
    a = np.ones((rows, cols), np.int8)
    for r in range(rows):
        for c in range(cols):
            b = a.copy()
            b[r, c] = -1  # one single-site cluster rooted at (r, c)
            a2, _ = twin.move(a, b, False, seed, m, slot)
            w = twin.philox4x32_10(c >> 2, r, m, 9 | (slot << 8), seed & 0xFFFFFFFF, seed >> 32)
            assert bool(a2[r, c] == -1) == bool(int(w[c & 3]) >> 31)


def test_ladder_twin_places_the_pass():
    """every = 2, t_max between the temperatures: passes in rounds 0, 2, 4 at the cold slots only, after the sweeps."""
    rows, cols, R = 6, 8, 4
    rng = np.random.default_rng(1)
    dis = _dyadic(rows, cols, True, rng)
    T = [0.5, 1.0, 2.0, 4.0]
    spins = [[rng.choice([-1, 1], size=(rows, cols)).astype(np.int8) for _ in range(R)] for _ in range(2)]
    lad = twin.Ladders(spins, True, dis, T, 11, every=2, t_max=1.5)
    plain = twin.tempering_twin.Ladders(spins, True, dis, T, 11)

    def energies_of(obj):
        return lambda j, k: np.array([dtwin.energy(obj.spins[k][w], True, *dis) for w in range(R)])
    out = lad.run(5, 1, True, True, energies_of(lad))
    ref = plain.run(5, 1, True, True, energies_of(plain))
    assert lad.passes == 3 and (lad.slot_passes == np.array([3, 3, 0, 0])).all()
    assert out["q"].shape == ref["q"].shape == (5, R)
    off = twin.Ladders(spins, True, dis, T, 11)  # every = 0 is the parent
    got = off.run(5, 1, True, True, energies_of(off))
    for key in ref:
        assert np.array_equal(got[key], ref[key]), key


def _exact(jr, jd, Ts):
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
            E -= float(jr[r, c]) * (S[:, n] * S[:, r * cols + (c + 1) % cols])
            E -= float(jd[r, c]) * (S[:, n] * S[:, ((r + 1) % rows) * cols + c])
    out = []
    for T in Ts:
        w = np.exp(-(E - E.min()) / T)
        w /= w.sum()
        Sf = S.astype(np.float64)
        C = Sf.T @ (Sf * w[:, None])
        out.append((float(w @ E) / N, float((C ** 2).sum()) / N ** 2))
    return out


def test_twin_equilibrium_against_exact_enumeration():
    """4 x 4 periodic +-J at T = 0.6: two replicas, one twin sweep + one pass per step; <E>/N and <q^2> within 4 s.e. + 1e-4 of
    exact enumeration over 20 batches (the rule of the tempering test)."""
    rows = cols = 4
    N, T, seed = 16, 0.6, 2024
    rng = np.random.default_rng(4)
    jr = rng.choice([-1.0, 1.0], size=(rows, cols)).astype(np.float32)
    jd = rng.choice([-1.0, 1.0], size=(rows, cols)).astype(np.float32)
    a = rng.choice([-1, 1], size=(rows, cols)).astype(np.int8)
    b = rng.choice([-1, 1], size=(rows, cols)).astype(np.int8)
    n_steps, nb, burn = 6000, 20, 200
    e, q2 = np.zeros(n_steps), np.zeros(n_steps)
    for t in range(burn + n_steps):
        a = dtwin.sweep(a, True, jr, jd, None, T, 1, seed, t, 0)
        b = dtwin.sweep(b, True, jr, jd, None, T, 1, seed + 1, t, 0)
        a, b = twin.move(a, b, True, seed, t, 0)
        if t >= burn:
            e[t - burn] = 0.5 * (dtwin.energy(a, True, jr, jd, None) + dtwin.energy(b, True, jr, jd, None)) / N
            q2[t - burn] = (dtwin.overlap(a, b) / N) ** 2
    (e_ex, q2_ex), = _exact(jr, jd, [T])
    for series, ex in ((e, e_ex), (q2, q2_ex)):
        bm = series.reshape(nb, -1).mean(axis=1)
        se = bm.std(ddof=1) / math.sqrt(nb)
        print(f"mean={bm.mean():+.6f} exact={ex:+.6f} se={se:.2e}")
        assert abs(bm.mean() - ex) < 4 * se + 1e-4, (bm.mean(), ex, se)


# ---------------------------------------------------------------- validation before the device is touched
@pytest.fixture
def no_device(monkeypatch):
    from tsu import _hip

    def boom(*a, **k):
        raise AssertionError("the device was touched before validation")
    monkeypatch.setattr(_hip, "TemperingLattice", boom)
    monkeypatch.setattr(_hip, "Lattice", boom)
    return _hip


@pytest.mark.parametrize("kw", [
    dict(cluster_moves=1, ladders=1),
    dict(cluster_moves=1),  # ladders defaults to 1
    dict(cluster_moves=-1, ladders=2),
    dict(cluster_moves=1.5, ladders=2),
    dict(cluster_moves="1", ladders=2),
    dict(cluster_moves=True, ladders=2),
    dict(cluster_moves=1, ladders=2, cluster_max_temperature=0.0),
    dict(cluster_moves=1, ladders=2, cluster_max_temperature=-2.0),
    dict(cluster_moves=1, ladders=2, cluster_max_temperature=float("nan")),
    dict(cluster_moves=1, ladders=2, cluster_max_temperature="warm"),
    dict(cluster_moves=0, ladders=2, cluster_max_temperature=0.0),
])
def test_cluster_move_validation_precedes_device(no_device, kw):
    from tsu.models.ising import LatticeTempering
    with pytest.raises(ValueError):
        LatticeTempering(8, [0.5, 1.0, 2.0], seed=1, **kw)


def test_tempering_scan_validation_precedes_device(no_device):
    from tsu.models.ising import tempering_scan
    with pytest.raises(ValueError, match="ladders=2"):
        tempering_scan(8, [1.0, 2.0], cluster_moves=1)
    with pytest.raises(ValueError):
        tempering_scan(8, [1.0, 2.0], replicas=2, cluster_moves=-3)
    with pytest.raises(ValueError):
        tempering_scan(8, [1.0, 2.0], replicas=2, cluster_moves=1, cluster_max_temperature=0)


def test_symbols_in_header_and_library():
    from tsu import _hip
    header = open(os.path.join(ROOT, "include", "tsu_hip.h")).read()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for n in ICM_SYMBOLS:
        assert re.search(rf"\b{n}\s*\(", header), n
        assert hasattr(lib, n), n
        assert n in _hip.SIGNATURES, n
    common = open(os.path.join(ROOT, "tsu-emulator_amd", "csrc", "tsu_common.h")).read()
    assert re.search(r"TSU_TAG_PT_ICM\s*=\s*9\b", common) and twin.TAG_PT_ICM == 9
    for name in ("set_cluster_moves", "cluster_move", "cluster_stats"):
        assert hasattr(_hip.TemperingLattice, name), name

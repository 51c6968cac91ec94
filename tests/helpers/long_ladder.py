"""What the long-ladder tests share (tests/test_long_ladders_cpu.py, tests/test_long_ladders_gpu.py): tempering ladders of 65 to 256
temperatures, rehearsed on the CPU with no device.

  dyadic_disorder   couplings k / 8 with k in [-8, 8] and fields k / 8 with k in [-4, 4], float32, bonds across an open boundary 0: every
                    energy term is a small multiple of 1 / 8, so the float64 energy is exact in ANY summation order.  The device's
                    fixed-order sums then equal the twins' `energy` with ==, the twins run on their own energies, and every swap
                    decision of a run is known before a device sees it.
  temperatures      np.geomspace(0.3, 4.0, R)
  start             the device's random start of walker g (the lattice's randomize(seed + g)), from population_twin.initial_spins
  conveyor          with bit-equal energies every delta of the sequential swap pass is +-0 and every pair is accepted: one pass carries
                    the walker at slot 0 to slot R - 1 and shifts the others down by one.  The closed form of the tables after n passes.
  lattice_run / icm_run / sparse_run
                    the twins' runs of the cases the two test files share, each computed once per process (the CPU file asserts the
                    coverage conditions on them, the GPU file compares the device with them)
"""
import functools
import importlib.util
import os

import numpy as np


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


population_twin = _load("population_twin")
tempering_twin = _load("tempering_twin")
tempering3d_twin = _load("tempering3d_twin")
icm_twin = _load("icm_twin")
overlap_twin = _load("overlap_twin")
correlation_twin = _load("correlation_twin")
disorder_twin = tempering_twin.disorder_twin
lattice3d_twin = tempering3d_twin.lattice3d_twin

LADDER_SEED, DISORDER_SEED = 77, 3

# section A: (shape, periodic, ladders, R); every case runs RUNS with ladder seed 77 on dyadic disorder of seed 3
LATTICE_CASES = [((6, 10), True, 2, 256), ((5, 37), False, 1, 129), ((6, 10), True, 2, 65), ((6, 10), True, 1, 64),
                 ((3, 5, 9), False, 2, 130), ((4, 4, 8), True, 1, 256)]
RUNS = ((4, 2), (3, 1))
# section C: two ladders of 130 temperatures, three rounds of two sweeps, one round at a time
SLOT_PASS_CASES = [((8, 16), True, 2, 130), ((3, 4, 16), (False, True, True), 2, 130)]
# section D: 100 of 130 slots take part in the cluster moves
ICM_SHAPE, ICM_R, ICM_SLOTS = (12, 16), 130, 100
# section F
SPARSE_ROUNDS, SPARSE_INTERVAL, SPARSE_SEED = 6, 2, 42


def axes(shape, periodic):
    return (bool(periodic),) * len(shape) if isinstance(periodic, (bool, np.bool_)) else tuple(bool(p) for p in periodic)


def dyadic_disorder(shape, periodic, seed):
    """(J_right, J_down, h) of a 2-D shape, (J_right, J_down, J_layer, h) of a 3-D one: J = integers(-8, 9) / 8, then h =
    integers(-4, 5) / 8, float32; the couplings along an open axis are 0 at its last index."""
    rng = np.random.default_rng(seed)
    nd = len(shape)
    js = [(rng.integers(-8, 9, size=shape) / 8).astype(np.float32) for _ in range(nd)]
    h = (rng.integers(-4, 5, size=shape) / 8).astype(np.float32)
    per = axes(shape, periodic)
    for j, a in enumerate(js):  # js[j]: the bonds along axis nd - 1 - j (J_right first)
        axis = nd - 1 - j
        if not per[axis]:
            a[(slice(None),) * axis + (-1,)] = 0.0
    return tuple(js) + (h,)


def zero_disorder(shape):
    """All couplings 0 and no field: every energy is 0 (section B)."""
    return tuple(np.zeros(shape, np.float32) for _ in shape) + (None,)


def temperatures(R):
    return np.geomspace(0.3, 4.0, R)


def sparse_temperatures(R):
    """Section F.  oracle.dyadic_system draws couplings of at most 3 / 128 and biases of at most 12 / 128, a sixteenth of the lattices'
    k / 8: at temperatures(R) itself every delta of the swap pass is so small that a pair is all but never refused (0 to 4 refusals
    in the 3060 attempts of a run, rehearsed for five seeds).  The same ladder in units of the couplings: temperatures(R) / 16."""
    return temperatures(R) / 16.0


def start(shape, seed, n_walkers):
    """(n_walkers, *shape) int8: the device's random start of walker g = ladder R + w, the lattice's randomize(seed + g)."""
    return population_twin.initial_spins(tuple(shape), seed, n_walkers)


def energy(spins, periodic, dis):
    """The twins' float64 energy of a 2-D or 3-D plane."""
    if len(dis) == 3:
        return disorder_twin.energy(spins, periodic, *dis)
    return lattice3d_twin.energy(spins, periodic, *dis)


def energy_terms(spins, periodic, dis):
    """Every term of -E, bond by bond and site by site, as one flat float64 array (for the order-independence check)."""
    s = np.asarray(spins, dtype=np.float64)
    per = axes(s.shape, periodic)
    nd = s.ndim
    out = []
    for j, J in enumerate(dis[:nd]):
        axis = nd - 1 - j
        t = np.asarray(J, dtype=np.float64) * s * np.roll(s, -1, axis=axis)
        if not per[axis]:
            t = np.delete(t, s.shape[axis] - 1, axis=axis)
        out.append(t.ravel())
    if dis[nd] is not None:
        out.append((np.asarray(dis[nd], dtype=np.float64) * s).ravel())
    return np.concatenate(out)


def conveyor(R, n):
    """The tables of one ladder after n passes in which every pair is accepted, from the identity start: walker_at_slot (R,),
    round_trips by walker (R,), accepts = attempts (R - 1,), and `rows` (n, R), the walker row recorded after each pass."""
    i = np.arange(R)
    return {"walker_at_slot": (i + n) % R, "round_trips": (n - i) // R, "accepts": np.full(R - 1, n, np.int64),
            "rows": (i[None, :] + np.arange(1, n + 1)[:, None]) % R}


def conveyor_rehearsal(R, splits):
    """tempering_twin.swap_pass with equal energies, sum(splits) passes: the same tables as `conveyor` returns."""
    was = np.arange(R)
    flags = np.full(R, tempering_twin.NONE)
    flags[0] = tempering_twin.BOTTOM
    trips, att, acc = np.zeros(R, np.int64), np.zeros(R - 1, np.int64), np.zeros(R - 1, np.int64)
    rows, t = [], 0
    for n in splits:  # a split run keeps its tables and its round counter
        for _ in range(n):
            tempering_twin.swap_pass(was, temperatures(R), np.zeros(R), tempering_twin.swap_uniforms(R, t, LADDER_SEED, 0), att, acc,
                                     flags, trips)
            rows.append(was.copy())
            t += 1
    return {"walker_at_slot": was, "round_trips": trips, "accepts": acc, "attempts": att, "rows": np.array(rows)}


# ---------------------------------------------------------------------------------------------------- the twins' runs, once each
def _ladders(shape, periodic, ladders, R, dis, seed, cls=None, **kw):
    s0 = start(shape, seed, ladders * R)
    spins = [[s0[k * R + w] for w in range(R)] for k in range(ladders)]
    if cls is None:
        cls = tempering_twin.Ladders if len(shape) == 2 else tempering3d_twin.Ladders
    return cls(spins, periodic, dis, temperatures(R), seed, **kw)


def _own_energies(tw):
    return lambda j, k: np.array([energy(s, tw.periodic, tw.disorder) for s in tw.spins[k]])


def _tables(tw):
    return {"attempts": tw.attempts.copy(), "accepts": tw.accepts.copy(), "round_trips": tw.trips.copy(),
            "walker_at_slot": tw.walker_at_slot.copy(), "sweep_count": tw.sweeps, "round_count": tw.rounds}


@functools.lru_cache(maxsize=None)
def lattice_run(shape, periodic, ladders, R):
    """Section A: the twin's record of RUNS on its own energies.  {"dis", "after": [(history, tables) per run], "spins": [k][w],
    "E": (nl, R) by walker}."""
    dis = dyadic_disorder(shape, periodic, DISORDER_SEED)
    tw = _ladders(shape, periodic, ladders, R, dis, LADDER_SEED)
    after = []
    for n, interval in RUNS:
        hist = tw.run(n, interval, True, True, _own_energies(tw))
        after.append((hist, _tables(tw)))
    E = np.array([[energy(s, periodic, dis) for s in lad] for lad in tw.spins])
    return {"dis": dis, "after": after, "spins": tw.spins, "E": E}


@functools.lru_cache(maxsize=None)
def slot_pass_run(shape, periodic, ladders, R):
    """Section C: three recorded rounds of two sweeps; per round the planes at every slot of both ladders and the twins' q, q_link
    and modes of the pair there."""
    dis = dyadic_disorder(shape, periodic, DISORDER_SEED)
    tw = _ladders(shape, periodic, ladders, R, dis, LADDER_SEED)
    per = np.array(axes(shape, periodic))
    overlap = disorder_twin.overlap if len(shape) == 2 else lattice3d_twin.overlap
    rows = {"walker": [], "q": [], "q_link": [], "modes": []}
    for _ in range(3):
        hist = tw.run(1, 2, True, True, _own_energies(tw))
        rows["walker"].append(hist["walker"][0])
        q, L, F = [], [], []
        for i in range(R):
            a, b = tw.spins[0][tw.walker_at_slot[0, i]], tw.spins[1][tw.walker_at_slot[1, i]]
            q.append(overlap(a, b))
            L.append(overlap_twin.link_overlap(a, b, periodic)[0])
            F.append(correlation_twin.modes(correlation_twin.profiles(a, b), tuple(per))[per])
        rows["q"].append(q)
        rows["q_link"].append(L)
        rows["modes"].append(F)
        assert (hist["q"][0] == np.array(q)).all()
    return {"dis": dis, "walker": np.array(rows["walker"]), "q": np.array(rows["q"], np.int64),
            "q_link": np.array(rows["q_link"], np.int64), "modes": np.array(rows["modes"], np.complex128), "tables": _tables(tw)}


def icm_t_max():
    T = temperatures(ICM_R)
    return float(np.sqrt(T[ICM_SLOTS - 1] * T[ICM_SLOTS]))


@functools.lru_cache(maxsize=None)
def icm_run():
    """Section D: three rounds of two sweeps with a cluster pass in every round over the slots below t_max, on its own energies."""
    dis = dyadic_disorder(ICM_SHAPE, True, DISORDER_SEED)
    tw = _ladders(ICM_SHAPE, True, 2, ICM_R, dis, LADDER_SEED, cls=icm_twin.Ladders, every=1, t_max=icm_t_max())
    hist = tw.run(3, 2, True, True, _own_energies(tw))
    E = np.array([[energy(s, True, dis) for s in lad] for lad in tw.spins])
    return {"dis": dis, "hist": hist, "tables": _tables(tw), "spins": tw.spins, "E": E, "passes": tw.passes,
            "slot_passes": tw.slot_passes.copy(), "clusters": tw.clusters.copy(), "flipped": tw.flipped.copy()}


def sparse_dyadic(n, seed):
    """test_sparse_batch_gpu._dyadic by value: a sparse system whose energies are exact in every summation order."""
    import scipy.sparse as sp
    from oracle import oracle as ora
    from tsu.graph import canonical_csr
    J, b, _ = ora.dyadic_system(n, seed)
    keep = np.triu(np.random.default_rng(seed).random((n, n)) < min(1.0, 6.0 / n))
    A = canonical_csr(sp.csr_matrix(J * (keep | keep.T)))
    assert ora.energy_is_exact(A.toarray(), b)
    return A, b


@functools.lru_cache(maxsize=None)
def sparse_run(R):
    """Section F: sparse_batch_twin.Batch on sparse_dyadic(64, 9), two ladders, SPARSE_ROUNDS rounds of SPARSE_INTERVAL sweeps, on its
    own energies.  (E, M, walker, batch)."""
    from tsu.graph import color_graph
    sbt = _load("sparse_batch_twin")
    A, bias = sparse_dyadic(64, 9)
    _, order = color_graph(A)
    b = sbt.Batch(A, bias, order, sparse_temperatures(R), ladders=2, seed=SPARSE_SEED)
    E, M, W = b.run(SPARSE_ROUNDS, SPARSE_INTERVAL)
    return E, M, W, b


# ---------------------------------------------------------------------------------------------------- the coverage conditions
def both_outcomes(attempts, accepts):
    """bool per pair: it has an accepted and a refused attempt."""
    return (accepts > 0) & (accepts < attempts)


def coverage(attempts, accepts, walker_at_slot):
    """Per ladder: (pairs >= 64 with both outcomes, pairs < 64 with both outcomes, the fraction of the slots >= 64 that hold a walker
    other than their own)."""
    out = []
    for k in range(attempts.shape[0]):
        both = both_outcomes(attempts[k], accepts[k])
        R = walker_at_slot.shape[1]
        moved = walker_at_slot[k, 64:] != np.arange(64, R)
        out.append((int(both[64:].sum()), int(both[:64].sum()), float(moved.mean()) if moved.size else 0.0))
    return out

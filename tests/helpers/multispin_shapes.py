"""The one table of cases of tests/test_multispin_full_size_gpu.py and tests/test_multispin_full_size_cpu.py: K9 at shapes that split
every grid of csrc/multispin.hip and csrc/multispin_pt.hip, and what the NumPy twins make of them.  Everything here runs on the CPU;
the device test compares with it word for word, the CPU test asserts what the inputs must hold for that comparison to mean something
(ties, accepted and refused swaps, far-end results that differ from those at counter 0).

The start of every case is k9_randomize's: every sample of plane (t, a) takes tsu_ising3d_randomize(seeds[t][a])
(tempering3d_twin.initial_spins), so a word is all ones or zero.  The device test asserts that before the first sweep.
Seeds, swap seeds and counter positions come from tests/helpers/far_end.py.
"""
import copy
import importlib.util
import os

import numpy as np


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


pt_twin = _load("multispin_pt_twin")
msc = pt_twin.msc
lat3 = msc.lat3
fe = _load("far_end")
_init = _load("tempering3d_twin").initial_spins


def PICK(S):
    """The samples tied to the single lattice: both ends of word 0, the ends of word 1."""
    return (0, 63, 64, S - 1)


# ---------------------------------------------------------------------------------------------------------------- 1. sweeps
# name -> shape, periodic (z, r, c), S, temperatures, replicas, routes (None: auto), the two calls' sweeps, the first call's sweep0
SWEEPS = {
    # 2048 octets: 8 workgroups of k9_sweep per plane; k9_measure gets two workgroups and 64 sites per lane
    "cube32": dict(shape=(32, 32, 32), periodic=True, S=70, Ts=(0.7, 1.4), A=2, routes=("hbm",), calls=(3, 2), sweep0=0),
    # 65 octets per row, the last of 6 columns; 1040 octets: a fifth workgroup of 16 live octets and three dead waves; 16480 sites: a
    # second k9_measure workgroup of 96 live lanes
    "long_rows": dict(shape=(4, 4, 1030), periodic=(True, False, True), S=65, Ts=(1.1,), A=1, routes=("hbm",), calls=(3, 2), sweep0=0),
    # 2046 octets, 18414 sites, odd everything, missing bonds across workgroups
    "odd_open": dict(shape=(33, 31, 18), periodic=False, S=64, Ts=(0.9, 1.8), A=2, routes=("hbm",), calls=(3, 2), sweep0=0),
    # 8192 sites and 1024 octets: both bounds of the small route at once; the case at the far end of the sweep counter
    "small_limit": dict(shape=(16, 64, 8), periodic=True, S=70, Ts=(0.8, 1.6), A=2, routes=("small", "hbm", None), calls=(3, 2),
                        sweep0=fe.end(5)),
    # 8192 sites through 512 octets of 16 columns
    "small_wide": dict(shape=(8, 8, 128), periodic=True, S=64, Ts=(1.2,), A=1, routes=("small", "hbm"), calls=(3, 2), sweep0=0),
    # 65280 planes: the plane axis of every grid next to its limit of 65535
    "many_planes": dict(shape=(4, 4, 4), periodic=True, S=8192, Ts=tuple(np.linspace(0.5, 3.0, 255)), A=2, routes=("small", "hbm"),
                        calls=(1, 1), sweep0=0),
}
DISORDER_SEED = 41
# the other side of msc_fits_small: (shape, what exceeds)
TOO_LARGE_FOR_SMALL = (((16, 64, 10), "10240 sites"), ((18, 64, 4), "1152 octets"))

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def plane_seeds(n_temps, replicas, base=fe.SEED_HI):
    """seeds[t][a] = base + a n_temps + t, the models' default layout, from the far-end base."""
    return [[base + a * n_temps + t for a in range(replicas)] for t in range(n_temps)]


def couplings(shape, periodic, S, seed=DISORDER_SEED):
    """(the float arrays the models take, their packed words 'J = -1' by multispin_twin.pack)."""
    def make():
        from tsu.models import edwards_anderson_samples
        j = edwards_anderson_samples(shape, S, kind="bimodal", seed=seed, periodic=periodic)
        return j, [msc.pack(a == -1) for a in j]
    return cached(("j", tuple(shape), str(periodic), S, seed), make)


def start_planes(shape, seeds, W):
    """(n_temps, replicas, W, D, R, C) uint64: k9_randomize's planes for seeds[t][a]."""
    return np.stack([np.stack([np.broadcast_to(np.where(_init(shape, sd, 1)[0] == 1, msc.ALL, msc.ZERO), (W,) + tuple(shape))
                               for sd in row]) for row in seeds]).astype(np.uint64)


def sweep_case(name, sweep0=None):
    """The twin's run of SWEEPS[name] (from `sweep0`, by default the case's own): start, planes after both calls, the integers of
    measure(), and the count of hi16 ties."""
    c = SWEEPS[name]
    s0 = c["sweep0"] if sweep0 is None else sweep0

    def make():
        shape, per, S, Ts, A = c["shape"], c["periodic"], c["S"], c["Ts"], c["A"]
        W = (S + 63) // 64
        _, j = couplings(shape, per, S)
        seeds = plane_seeds(len(Ts), A)
        start = start_planes(shape, seeds, W)
        planes, stats = start.copy(), {}
        for t, T in enumerate(Ts):
            for a in range(A):
                planes[t, a] = msc.bitsliced_sweep(planes[t, a], per, *j, T, sum(c["calls"]), seeds[t][a], s0, stats)
        unsat, ssum, q, ql, nb = pt_twin.measure(planes, per, *j, S)
        return dict(start=start, planes=planes, unsat=unsat, sum=ssum, q=q, ql=ql, nb=nb, ties=stats.get("ties", 0), seeds=seeds)
    return cached(("sweeps", name, s0), make)


# ---------------------------------------------------------------------------------------------------------------- 2. measurement
MEASURE = {"cube32": ((32, 32, 32), True), "long_rows": ((4, 4, 1030), (True, False, True))}


def measure_case(name):
    """64 samples, one slot, two replicas, planes and couplings by construction (sample b by b % 4):
      0  all up in both replicas, every bond J = -1: every bond unsatisfied, unsat = N_b, sum = N, q = N, q_link = N_b
      1  replica 0 all up, replica 1 the checkerboard (z + r + c) & 1, J = +1: unsat = (0, N_b), q = 0, q_link = -N_b
      2  all down, J = +1: unsat = 0, sum = -N, q = N, q_link = N_b
      3  random spins and couplings
    Returns the float couplings, their packed words, the planes (1, 2, 1, D, R, C) and the closed forms."""
    shape, per = MEASURE[name]

    def make():
        from tsu.models.ising import lattice_bond_count
        rng = np.random.default_rng(77)
        N, nb = int(np.prod(shape)), lattice_bond_count(shape, per)
        board = lat3.colours(shape) == 1
        up = np.zeros((2, 64) + shape, bool)
        j = [np.ones((64,) + shape, np.float32) for _ in range(3)]
        for b in range(64):
            if b % 4 == 0:
                up[:, b] = True
                for a in j:
                    a[b] = -1.0
            elif b % 4 == 1:
                up[0, b] = True
                up[1, b] = board
            elif b % 4 == 3:
                up[:, b] = rng.integers(0, 2, size=(2,) + shape).astype(bool)
                for a in j:
                    a[b] = 2.0 * rng.integers(0, 2, size=shape) - 1.0
        for k, a in enumerate(j):  # array k holds the bonds along axis 2 - k; an open axis has no last bond
            if not lat3.axes(per)[2 - k]:
                idx = [slice(None)] * 4
                idx[3 - k] = -1
                a[tuple(idx)] = 0.0
        planes = np.stack([msc.pack(up[0]), msc.pack(up[1])])[None]
        closed = {0: dict(unsat=(nb, nb), sum=(N, N), q=N, ql=nb), 1: dict(unsat=(0, nb), sum=(N, 0), q=0, ql=-nb),
                  2: dict(unsat=(0, 0), sum=(-N, -N), q=N, ql=nb)}
        return dict(j=tuple(j), packed=[msc.pack(a == -1) for a in j], planes=planes, closed=closed, N=N, nb=nb)
    return cached(("measure", name), make)


# ---------------------------------------------------------------------------------------------------------------- 3. ladders
LADDER_SHAPE, LADDER_S, LADDER_A = (4, 4, 4), 70, 2
# n_temps -> routes: one pair; 8 and 9 pairs (k9_pt_apply's look-ahead); 16 and 17 (one chunk of k9_pt_plan, one pair into the
# second); 32 (two full chunks)
LADDERS = {2: (None,), 9: (None,), 10: (None,), 17: ("small", "hbm"), 18: ("small", "hbm"), 33: (None,)}
LADDER_ROUNDS, LADDER_K = 3, 1
CUBE32_TS, CUBE32_ROUNDS, CUBE32_K = (1.50, 1.51, 1.52), 4, 2  # at 32^3 a pair accepts only between temperatures this close


def swap_seeds(S, base=fe.SEED_CARRY):
    """base + s: with far_end.SEED_CARRY the carry into the high key word falls at sample 2."""
    return [base + s for s in range(S)]


class Run:
    """A Tempering twin and what it recorded, with snapshots: rows[r] = (unsat, sum, q, q_link) of round r."""

    def __init__(self, shape, periodic, S, Ts, A, sweeps0=0, rounds0=0):
        self.shape, self.periodic, self.S, self.Ts, self.A = shape, periodic, S, tuple(float(x) for x in Ts), A
        _, j = couplings(shape, periodic, S)
        self.seeds = plane_seeds(len(self.Ts), A)
        self.swap_seeds = swap_seeds(S)
        self.start = start_planes(shape, self.seeds, (S + 63) // 64)
        self.twin = pt_twin.Tempering(self.start, periodic, *j, self.Ts, self.seeds, self.swap_seeds, S)
        self.twin.sweeps, self.twin.book.rounds = sweeps0, rounds0
        self.rows, self.snap, self.masks = [], {}, []

    def run(self, n_rounds, interval):
        for _ in range(n_rounds):
            before = self.twin.book.accepts.copy()
            cols = self.twin.run(1, interval)
            self.rows.append(tuple(None if c is None else c[0] for c in cols))
            self.masks.append(self.twin.book.accepts - before)  # (A, S, R - 1) 0 / 1: this pass's accepts
        self.snap[len(self.rows)] = (self.twin.planes.copy(), copy.deepcopy(self.twin.book))
        return self

    def rows_of(self, first, n):
        return tuple(np.stack([r[k] for r in self.rows[first:first + n]]) for k in range(4))

    def mixed_mask_words(self):
        """How many (pass, pair, replica, word) mask words are neither 0 nor all the word's samples."""
        n = 0
        for m in self.masks:
            for w in range((self.S + 63) // 64):
                cnt = m[:, 64 * w:64 * w + 64].sum(axis=1)  # (A, R - 1)
                n += int(np.count_nonzero((cnt > 0) & (cnt < min(64, self.S - 64 * w))))
        return n


def ladder_run(n_temps):
    return cached(("ladder", n_temps), lambda: Run(LADDER_SHAPE, True, LADDER_S, np.linspace(0.5, 2.5, n_temps), LADDER_A)
                  .run(LADDER_ROUNDS, LADDER_K))


def cube32_ladder_run():
    c = SWEEPS["cube32"]
    return cached(("ladder", "cube32"), lambda: Run(c["shape"], c["periodic"], c["S"], CUBE32_TS, c["A"]).run(CUBE32_ROUNDS, CUBE32_K))


# ---------------------------------------------------------------------------------------------------------------- 4. and 5.
# the cube and open_rows cases of tests/test_multispin_pt_gpu.py
PT_CASES = {"cube": ((4, 4, 6), True), "open_rows": ((4, 5, 18), (True, False, True))}
PT_S, PT_TS, PT_A = 70, (0.6, 0.9, 1.3, 1.8, 2.5), 2
RING_STOPS = (5, 7, 66, 77, 86, 131)  # rounds after which the ring tests look: see test_multispin_full_size_gpu.py


def ring_run():
    """131 rounds of one sweep on the cube, snapshots at RING_STOPS."""
    def make():
        shape, per = PT_CASES["cube"]
        r, done = Run(shape, per, PT_S, PT_TS, PT_A), 0
        for stop in RING_STOPS:
            r.run(stop - done, 1)
            done = stop
        return r
    return cached(("ring",), make)


FAR_ROUNDS, FAR_K = 6, 2
FAR_POSITIONS = {"straddle": (fe.straddle(FAR_ROUNDS * FAR_K), fe.straddle32(FAR_ROUNDS)),
                 "end": (fe.end(FAR_ROUNDS * FAR_K), fe.end32(FAR_ROUNDS)), "zero": (0, 0)}


def far_run(name, position):
    shape, per = PT_CASES[name]
    s0, r0 = FAR_POSITIONS[position]
    return cached(("far", name, position), lambda: Run(shape, per, PT_S, PT_TS, PT_A, s0, r0).run(FAR_ROUNDS, FAR_K))

"""NumPy twin of K7 parallel tempering (tsu_pt2d_*, csrc/ising2d_disorder.hip), bit for bit given the walkers' energies.

Contract ("Parallel tempering (K7)"), ladder k of R walkers on one disorder:
  walker w of ladder k: a K7 lattice with key seed + k R + w, replica 0, the shared sweep counter; it starts at slot w
  round: swap_interval K7 sweeps of every walker at the temperature of its slot, every energy, one swap pass per ladder, the record
  swap pass (the reference's rule, gibbs.py:309-323): for i = 0 .. R-2 in order, a / b = the walkers at slots i / i + 1,
        delta = (1.0 / T_i - 1.0 / T_{i+1}) * (E_a - E_b); accept iff delta >= 0 or u_i < exp(delta); an accepted pair exchanges
        the walkers' slots (the reference writes E_b - E_a, the inverse of the detailed-balance ratio).  u_i = dense_uniform's 53-bit uniform of Philox(i >> 1, 0, t, TAG_PT_SWAP | k << 8), key = seed,
        t = the round counter
  round trips: a walker reaching slot 0 becomes BOTTOM (the walker starting there starts so), a BOTTOM walker reaching slot R - 1
        becomes TOP, a TOP walker reaching slot 0 counts one round trip
The sweeps are disorder_twin's; the energies are fed in (the device's fixed-order sums), so the swap decisions are the device's.
"""
import importlib.util
import os

import numpy as np


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


disorder_twin = _load("disorder_twin")
philox4x32_10 = _load("cluster_twin").philox4x32_10

TAG_DENSE = 4
TAG_PT_SWAP = 8
NONE, BOTTOM, TOP = 0, 1, 2


def uniform53(i, t, tag, seed):
    """dense_uniform (csrc/dense.h): the 53-bit uniform of index i from Philox(i >> 1, 0, t, tag), key = seed."""
    i = np.asarray(i, dtype=np.uint64)
    w = philox4x32_10(i >> np.uint64(1), 0, int(t), int(tag), int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    odd = (i & np.uint64(1)).astype(bool)
    a = np.where(odd, w[2], w[0]) >> np.uint32(5)
    b = np.where(odd, w[3], w[1]) >> np.uint32(6)
    return (a.astype(np.float64) * 67108864.0 + b.astype(np.float64)) / 9007199254740992.0


def swap_uniforms(R, t, seed, ladder):
    """u_i of the R - 1 pairs of ladder `ladder` in round t."""
    return uniform53(np.arange(R - 1), t, TAG_PT_SWAP | (int(ladder) << 8), seed)


def arrive(flags, trips, w, slot, R):
    """Round-trip bookkeeping of walker w arriving at `slot` (in place)."""
    if slot == 0:
        if flags[w] == TOP:
            trips[w] += 1
        flags[w] = BOTTOM
    elif slot == R - 1 and flags[w] == BOTTOM:
        flags[w] = TOP


def swap_pass(walker_at_slot, T, E, u, attempts, accepts, flags, trips):
    """One pass over the adjacent pairs of one ladder, in place.  E[w]: energy of walker w; T[i]: temperature of slot i."""
    R = len(walker_at_slot)
    for i in range(R - 1):
        a, b = int(walker_at_slot[i]), int(walker_at_slot[i + 1])
        delta = (1.0 / float(T[i]) - 1.0 / float(T[i + 1])) * (float(E[a]) - float(E[b]))
        attempts[i] += 1
        if delta >= 0 or u[i] < np.exp(delta):
            accepts[i] += 1
            walker_at_slot[i], walker_at_slot[i + 1] = b, a
            arrive(flags, trips, a, i + 1, R)
            arrive(flags, trips, b, i, R)


class Ladders:
    """The whole state: spins[k][w], walker_at_slot (nl, R), flags, trips (nl, R), attempts / accepts (nl, R - 1), counters."""

    def __init__(self, spins, periodic, disorder, T, seed):
        self.spins = [[np.array(s, np.int8) for s in lad] for lad in spins]
        self.nl, self.R = len(spins), len(T)
        self.periodic, self.disorder, self.T, self.seed = periodic, disorder, [float(x) for x in T], int(seed)
        self.walker_at_slot = np.tile(np.arange(self.R), (self.nl, 1))
        self.flags = np.full((self.nl, self.R), NONE)
        self.flags[:, 0] = BOTTOM
        self.trips = np.zeros((self.nl, self.R), np.int64)
        self.attempts = np.zeros((self.nl, self.R - 1), np.int64)
        self.accepts = np.zeros((self.nl, self.R - 1), np.int64)
        self.sweeps = self.rounds = 0

    def run(self, n_rounds, interval, swap, record, energies):
        """energies(j, k) -> E by walker of ladder k in round j of this run.  Returns the recorded rows like
        TemperingLattice.history(): E, M, walker (n, nl, R) and q (n, R) or None."""
        jr, jd, h = self.disorder
        rows = {"E": [], "M": [], "walker": [], "q": []}
        for j in range(n_rounds):
            for k in range(self.nl):
                for w in range(self.R):
                    T = self.T[int(np.flatnonzero(self.walker_at_slot[k] == w)[0])]
                    self.spins[k][w] = disorder_twin.sweep(self.spins[k][w], self.periodic, jr, jd, h, T, interval,
                                                           self.seed + k * self.R + w, self.sweeps, 0)
            self.sweeps += interval
            Es = [np.asarray(energies(j, k)) for k in range(self.nl)] if (swap or record) else None
            if swap:
                for k in range(self.nl):
                    swap_pass(self.walker_at_slot[k], self.T, Es[k], swap_uniforms(self.R, self.rounds, self.seed, k),
                              self.attempts[k], self.accepts[k], self.flags[k], self.trips[k])
            if record:
                was = self.walker_at_slot.copy()
                rows["walker"].append(was)
                rows["E"].append([[Es[k][was[k, i]] for i in range(self.R)] for k in range(self.nl)])
                rows["M"].append([[int(self.spins[k][was[k, i]].sum(dtype=np.int64)) for i in range(self.R)]
                                  for k in range(self.nl)])
                if self.nl == 2:
                    rows["q"].append([disorder_twin.overlap(self.spins[0][was[0, i]], self.spins[1][was[1, i]])
                                      for i in range(self.R)])
            self.rounds += 1
        n = n_rounds if record else 0
        return {"E": np.array(rows["E"], np.float64).reshape(n, self.nl, self.R),
                "M": np.array(rows["M"], np.int64).reshape(n, self.nl, self.R),
                "walker": np.array(rows["walker"], np.int32).reshape(n, self.nl, self.R),
                "q": np.array(rows["q"], np.int64).reshape(n, self.R) if self.nl == 2 else None}

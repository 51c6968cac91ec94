"""NumPy / oracle twin of a K5 walker batch (tsu_sparse_batch_*, csrc/sparse_batch.hip): the whole contract of DESIGN.md section 3,
"Walker batches on a sparse graph".

  walker g = ladder R + w starts at slot w; one sweep counter for all walkers, 0 after init
  sweep of walker g: ora.sparse_sweep_philox(state, graph, T of its slot, 1, seed, sweep, replica=g) in the colour-major order
  random start: bit i of walker g = [uniform53(i, 0, TAG_INIT | g << 8, seed) < 0.5]
  round: `interval` sweeps, the energies (if the round swaps, records or tracks best states), the best-state update, the swap pass
  swap pass: tempering_twin.swap_pass with tempering_twin.swap_uniforms(R, round, seed, ladder)
  energy: fixed_order_energy below
  best state: after each energy pass, walker g keeps the state and the energy if E_g < best_g (strict); the states a tracked run
        starts from are candidates
The energies may be fed in (the device's), so that the swap decisions are the device's.
"""
import importlib.util
import os

import numpy as np

from oracle import oracle as ora


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


tempering_twin = _load("tempering_twin")
uniform53, swap_pass, swap_uniforms = tempering_twin.uniform53, tempering_twin.swap_pass, tempering_twin.swap_uniforms

TAG_INIT = 2
LANES, SEGMENT = 1024, 65536


def fields(state, A):
    """F_i = sum over row i of A (CSR order, one IEEE addition per edge) of val * bit, for every site."""
    rp, ci, va = A.indptr, A.indices, A.data
    deg = np.diff(rp)
    b = np.asarray(state, dtype=np.float64)
    F = np.zeros(A.shape[0])
    for k in range(int(deg.max()) if deg.size else 0):
        rows = np.flatnonzero(deg > k)
        e = rp[rows] + k
        F[rows] = F[rows] + va[e] * b[ci[e]]
    return F


def fixed_order_energy(state, A, bias, order):
    """The batch's energy: terms e_p = -0.5 b F - bias b by POSITION p (site order[p]); per segment of 65536 positions the 1024
    strided partials P_j (p = j mod 1024, ascending) reduced by the halving tree P_j += P_{j+s}, s = 512 .. 1; the segments' sums
    added in ascending order."""
    order = np.asarray(order)
    b = np.asarray(state, dtype=np.float64)
    bias = np.zeros(b.size) if bias is None else np.asarray(bias, dtype=np.float64)
    terms = (-0.5 * b * fields(state, A) - bias * b)[order]
    total = 0.0
    for s0 in range(0, terms.size, SEGMENT):
        seg = terms[s0:s0 + SEGMENT]
        rows = -(-seg.size // LANES)
        pad = np.zeros(rows * LANES)
        pad[:seg.size] = seg
        pad = pad.reshape(rows, LANES)
        P = np.zeros(LANES)
        for r in range(rows):
            P = P + pad[r]
        s = LANES // 2
        while s >= 1:
            P[:s] = P[:s] + P[s:2 * s]
            s //= 2
        total = total + float(P[0])
    return total


def random_start(n, g, seed):
    return (uniform53(np.arange(n), 0, TAG_INIT | (int(g) << 8), seed) < 0.5).astype(np.int8)


class Batch:
    """states[g] (site order), walker_at_slot / flags / trips (nl, R), attempts / accepts (nl, R - 1), counters, best states."""

    def __init__(self, A, bias, order, T, ladders=1, seed=0, initial="random", track_best=False):
        self.A, self.bias, self.order = A, None if bias is None else np.asarray(bias, dtype=np.float64), np.asarray(order, dtype=np.int32)
        self.n, self.R, self.nl, self.seed = A.shape[0], len(T), int(ladders), int(seed)
        self.nw = self.R * self.nl
        self.T = [float(x) for x in T]
        if isinstance(initial, str):
            make = {"random": lambda g: random_start(self.n, g, seed), "zeros": lambda g: np.zeros(self.n, np.int8),
                    "ones": lambda g: np.ones(self.n, np.int8)}[initial]
            self.states = [make(g) for g in range(self.nw)]
        else:
            self.states = [np.array(s, np.int8) for s in initial]
        self.walker_at_slot = np.tile(np.arange(self.R), (self.nl, 1))
        self.flags = np.full((self.nl, self.R), tempering_twin.NONE)
        self.flags[:, 0] = tempering_twin.BOTTOM
        self.trips = np.zeros((self.nl, self.R), np.int64)
        self.attempts = np.zeros((self.nl, max(self.R - 1, 0)), np.int64)
        self.accepts = np.zeros((self.nl, max(self.R - 1, 0)), np.int64)
        self.sweeps = self.rounds = 0
        self.track = bool(track_best)
        self.best_E = np.full(self.nw, np.inf)
        self.best_states = [np.zeros(self.n, np.int8) for _ in range(self.nw)]
        self.pending = True

    def own_energies(self):
        return np.array([fixed_order_energy(s, self.A, self.bias, self.order) for s in self.states])

    def slot_of(self, g):
        k, w = divmod(g, self.R)
        return int(np.flatnonzero(self.walker_at_slot[k] == w)[0])

    def _candidates(self, E):
        for g in range(self.nw):
            if E[g] < self.best_E[g]:
                self.best_E[g] = E[g]
                self.best_states[g] = self.states[g].copy()

    def run(self, n_rounds, interval, swap=True, record=True, energies=None):
        """energies(j, batch) -> E by walker (nw,) in round j of this run (None: fixed_order_energy).  Returns the rows E, M, walker
        (rounds, nl, R) like SparseBatch.history()."""
        A = self.A
        rows = {"E": [], "M": [], "walker": []}
        if self.track and self.pending and n_rounds > 0:
            self._candidates(self.own_energies())
            self.pending = False
        for j in range(n_rounds):
            for g in range(self.nw):
                self.states[g] = ora.sparse_sweep_philox(self.states[g], A.indptr, A.indices, A.data, self.bias, self.T[self.slot_of(g)],
                                                         interval, self.seed, sweep0=self.sweeps, replica=g, order=self.order)
            self.sweeps += interval
            E = None
            if swap or record or self.track:
                E = np.asarray(energies(j, self) if energies is not None else self.own_energies(), dtype=np.float64).reshape(self.nl, self.R)
            if self.track:
                self._candidates(E.reshape(-1))
            if swap:
                for k in range(self.nl):
                    swap_pass(self.walker_at_slot[k], self.T, E[k], swap_uniforms(self.R, self.rounds, self.seed, k), self.attempts[k],
                              self.accepts[k], self.flags[k], self.trips[k])
            if record:
                was = self.walker_at_slot.copy()
                rows["walker"].append(was)
                rows["E"].append([[E[k][was[k, i]] for i in range(self.R)] for k in range(self.nl)])
                rows["M"].append([[int((2 * self.states[k * self.R + was[k, i]].astype(np.int64) - 1).sum()) for i in range(self.R)]
                                  for k in range(self.nl)])
            self.rounds += 1
        m = n_rounds if record else 0
        return (np.array(rows["E"], np.float64).reshape(m, self.nl, self.R), np.array(rows["M"], np.int64).reshape(m, self.nl, self.R),
                np.array(rows["walker"], np.int32).reshape(m, self.nl, self.R))

    def anneal(self, schedule, sweeps_per_step=1):
        """One temperature per step for every slot, or a row of R per step; each step one round without swaps."""
        S = np.asarray(schedule, dtype=np.float64)
        if S.ndim == 1:
            S = np.repeat(S[:, None], self.R, axis=1)
        for row in S:
            self.T = [float(x) for x in row]
            self.run(1, sweeps_per_step, swap=False, record=False)

    def state_at(self, slot, ladder=0):
        return self.states[ladder * self.R + int(self.walker_at_slot[ladder, slot])]

    def best(self):
        """(bits, energy): the first minimum in walker order."""
        g = int(np.argmin(self.best_E))
        return self.best_states[g], float(self.best_E[g])

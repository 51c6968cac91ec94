"""NumPy twin of K8 parallel tempering (tsu_pt3d_*, csrc/ising3d.hip), bit for bit given the walkers' energies.

Contract ("Parallel tempering in 3-D (K8)"), ladder k of R walkers on one disorder:
  walker w of ladder k: a K8 lattice with key seed + k R + w, replica 0, the shared sweep counter; it starts at slot w
  round: swap_interval K8 sweeps of every walker at the temperature of its slot, every energy, one swap pass per ladder, the record
  swap pass, uniforms and round-trip bookkeeping: the 2-D ladders' (tempering_twin.swap_pass / swap_uniforms / arrive), unchanged
The sweeps, energy and overlap are lattice3d_twin's.  The energies are fed in (the device's fixed-order sums), so the swap decisions
are the device's; with energies=None the twin uses its own float64 energies (a rehearsal of the statistics, not of the bits).
"""
import importlib.util
import os

import numpy as np


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


tempering_twin = _load("tempering_twin")
lattice3d_twin = _load("lattice3d_twin")
swap_pass, swap_uniforms, arrive = tempering_twin.swap_pass, tempering_twin.swap_uniforms, tempering_twin.arrive
NONE, BOTTOM, TOP = tempering_twin.NONE, tempering_twin.BOTTOM, tempering_twin.TOP
sweep, energy, overlap = lattice3d_twin.sweep, lattice3d_twin.energy, lattice3d_twin.overlap


def initial_spins(shape, seed, n_walkers, initial=0):
    """The start of walker g = 0 .. n_walkers - 1: tsu_ising3d_randomize(seed + g) (the bits of the 2-D randomize of a (D R) x C
    lattice, K1's: bit c & 15 of half (c >> 4) & 1 of Philox(c >> 7, rho, 0, TAG_INIT)[(c >> 5) & 3]), or all up / down."""
    D, R, C = shape
    if initial != 0:
        return [np.full(shape, initial, np.int8) for _ in range(n_walkers)]
    philox = tempering_twin.philox4x32_10
    rho, c = np.meshgrid(np.arange(D * R, dtype=np.uint64), np.arange(C, dtype=np.uint64), indexing="ij")
    out = []
    for g in range(n_walkers):
        s = int(seed) + g
        w = philox(c >> np.uint64(7), rho, 0, 2, s & 0xFFFFFFFF, (s >> 32) & 0xFFFFFFFF)
        word = np.choose(((c >> np.uint64(5)) & np.uint64(3)).astype(np.int64), [w[0], w[1], w[2], w[3]]).astype(np.uint64)
        bits = (word >> (np.uint64(16) * ((c >> np.uint64(4)) & np.uint64(1)))) & np.uint64(0xFFFF)
        bit = (bits >> (c & np.uint64(15))) & np.uint64(1)
        out.append(np.where(bit == 1, 1, -1).astype(np.int8).reshape(shape))
    return out


class Ladders:
    """The whole state: spins[k][w], walker_at_slot (nl, R), flags, trips (nl, R), attempts / accepts (nl, R - 1), counters.
    `disorder` = (J_right, J_down, J_layer, h or None); `periodic` a bool or a triple."""

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

    def run(self, n_rounds, interval, swap, record, energies=None):
        """energies(j, k) -> E by walker of ladder k in round j of this run (None: the twin's own float64 energies).  Returns the
        recorded rows like TemperingLattice3D.history(): E, M, walker (n, nl, R) and q (n, R) or None."""
        jr, jd, jl, h = self.disorder
        rows = {"E": [], "M": [], "walker": [], "q": []}
        for j in range(n_rounds):
            for k in range(self.nl):
                for w in range(self.R):
                    T = self.T[int(np.flatnonzero(self.walker_at_slot[k] == w)[0])]
                    self.spins[k][w] = sweep(self.spins[k][w], self.periodic, jr, jd, jl, h, T, interval,
                                             self.seed + k * self.R + w, self.sweeps, 0)
            self.sweeps += interval
            Es = None
            if swap or record:
                if energies is None:
                    Es = [np.array([energy(s, self.periodic, jr, jd, jl, h) for s in self.spins[k]]) for k in range(self.nl)]
                else:
                    Es = [np.asarray(energies(j, k)) for k in range(self.nl)]
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
                    rows["q"].append([overlap(self.spins[0][was[0, i]], self.spins[1][was[1, i]]) for i in range(self.R)])
            self.rounds += 1
        n = n_rounds if record else 0
        return {"E": np.array(rows["E"], np.float64).reshape(n, self.nl, self.R),
                "M": np.array(rows["M"], np.int64).reshape(n, self.nl, self.R),
                "walker": np.array(rows["walker"], np.int32).reshape(n, self.nl, self.R),
                "q": np.array(rows["q"], np.int64).reshape(n, self.R) if self.nl == 2 else None}

"""NumPy twin of K7's replica cluster moves (tsu_pt2d_cluster_move, csrc/ising2d_icm.hip), bit for bit.

One pass at slot i ("Replica cluster moves"), a / b = the walkers of ladder 0 / 1 now at that slot:
  q     q_x = a_x b_x; the sites with q = -1 are joined to their right and down lattice neighbours with q = -1 (wrapping on a
        periodic lattice, not on an open one), whatever J is on the bond; sites with q = +1 belong to no cluster
  root  the smallest index r * cols + c of a cluster
  flip  the cluster rooted at (r, c) flips in BOTH walkers iff bit 31 of word c & 3 of
        Philox4x32-10(c >> 2, r, m, TAG_PT_ICM | slot << 8) is set, key = the ladder's seed, m = the cluster-pass counter
The twin takes any shape (also those the device refuses: a wrap onto the same neighbour twice is one adjacency).
"""
import importlib.util
import os

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


tempering_twin = _load("tempering_twin")
disorder_twin = tempering_twin.disorder_twin
philox4x32_10 = tempering_twin.philox4x32_10

TAG_PT_ICM = 9


def roots(a, b, periodic):
    """(root index per site, -1 where q = +1) as a (rows, cols) int64 array."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    rows, cols = a.shape
    n = rows * cols
    neg = (a * b) < 0
    idx = np.arange(n, dtype=np.int64).reshape(rows, cols)
    ok_r = np.ones((rows, cols), bool)
    ok_d = np.ones((rows, cols), bool)
    if not periodic:
        ok_r[:, -1] = False
        ok_d[-1, :] = False
    act_r = ok_r & neg & np.roll(neg, -1, axis=1)
    act_d = ok_d & neg & np.roll(neg, -1, axis=0)
    src = np.concatenate([idx[act_r], idx[act_d]])
    dst = np.concatenate([np.roll(idx, -1, axis=1)[act_r], np.roll(idx, -1, axis=0)[act_d]])
    g = coo_matrix((np.ones(src.size, np.int8), (src, dst)), shape=(n, n))
    ncomp, lab = connected_components(g, directed=False)
    root = np.full(ncomp, n, dtype=np.int64)
    np.minimum.at(root, lab, np.arange(n, dtype=np.int64))
    out = root[lab].reshape(rows, cols)
    out[~neg] = -1
    return out


def move(a, b, periodic, seed, m, slot, stats=None):
    """One pass of the pair (a, b): returns the two new int8 arrays.  stats (a dict) receives `clusters` and `flipped`."""
    a, b = np.asarray(a, dtype=np.int8), np.asarray(b, dtype=np.int8)
    rows, cols = a.shape
    rt = roots(a, b, periodic)
    u = np.unique(rt[rt >= 0])
    flip = np.zeros((rows, cols), bool)
    if u.size:
        rr, rc = u // cols, u % cols
        w = philox4x32_10(rc >> 2, rr, int(m), TAG_PT_ICM | (int(slot) << 8), int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
        word = np.choose((rc & 3).astype(np.int64), w)
        flip_root = (word >> np.uint32(31)) == 1
        sel = rt >= 0
        flip[sel] = flip_root[np.searchsorted(u, rt[sel])]
    if stats is not None:
        stats["clusters"] = int(u.size)
        stats["flipped"] = int(flip.sum())
    return np.where(flip, -a, a).astype(np.int8), np.where(flip, -b, b).astype(np.int8)


class Ladders(tempering_twin.Ladders):
    """tempering_twin.Ladders with the pass inserted into the round: sweeps, the pass if one is due (round t of the handle with
    t % every == 0; the slots with T <= t_max), then energies, swap pass, record."""

    def __init__(self, spins, periodic, disorder, T, seed, every=0, t_max=np.inf):
        super().__init__(spins, periodic, disorder, T, seed)
        assert self.nl == 2 or every == 0
        self.every, self.t_max = int(every), float(t_max)
        self.passes = 0
        self.slot_passes = np.zeros(self.R, np.int64)
        self.clusters = np.zeros(self.R, np.int64)
        self.flipped = np.zeros(self.R, np.int64)

    def cluster_move(self):
        for i in range(self.R):
            if not self.T[i] <= self.t_max:
                continue
            wa, wb = int(self.walker_at_slot[0, i]), int(self.walker_at_slot[1, i])
            st = {}
            self.spins[0][wa], self.spins[1][wb] = move(self.spins[0][wa], self.spins[1][wb], self.periodic, self.seed,
                                                        self.passes, i, st)
            self.slot_passes[i] += 1
            self.clusters[i] += st["clusters"]
            self.flipped[i] += st["flipped"]
        self.passes += 1

    def run(self, n_rounds, interval, swap, record, energies):
        """The parent's round with the pass between the sweeps and the energies (the parent has no hook there, so its body is
        restated).  energies(j, k) -> E by walker of ladder k in round j of this run, AFTER that round's pass."""
        jr, jd, h = self.disorder
        rows = {"E": [], "M": [], "walker": [], "q": []}
        for j in range(n_rounds):
            for k in range(self.nl):
                for w in range(self.R):
                    T = self.T[int(np.flatnonzero(self.walker_at_slot[k] == w)[0])]
                    self.spins[k][w] = disorder_twin.sweep(self.spins[k][w], self.periodic, jr, jd, h, T, interval,
                                                           self.seed + k * self.R + w, self.sweeps, 0)
            self.sweeps += interval
            if self.every >= 1 and self.rounds % self.every == 0:
                self.cluster_move()
            Es = [np.asarray(energies(j, k)) for k in range(self.nl)] if (swap or record) else None
            if swap:
                for k in range(self.nl):
                    tempering_twin.swap_pass(self.walker_at_slot[k], self.T, Es[k],
                                             tempering_twin.swap_uniforms(self.R, self.rounds, self.seed, k),
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

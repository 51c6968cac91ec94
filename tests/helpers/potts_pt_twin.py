"""NumPy twin of K13, parallel tempering of K12's Potts lattice (tsu_potts_pt_*, csrc/potts_pt.hip), bit for bit given the walkers'
energies.

Contract ("Parallel tempering (K13)"), ladder k of R walkers on one disorder:
  walker g = k R + w: a K12 lattice (potts_disorder_twin) with key seed + g, replica 0, the shared sweep counter; it starts at slot w
        from default_rng(seed + g).integers(0, q, shape) or from one colour; the key travels with the walker, T belongs to the slot
  round: swap_interval K12 heat-bath sweeps of every walker at the temperature of its slot, every walker's n_eq, N_c and E, one swap
        pass per ladder (tempering_twin.swap_pass with tempering_twin.swap_uniforms: tag TAG_PT_SWAP | k << 8, key = seed, t = the
        round counter), then the record; with two ladders, per slot, the contingency table C[a][b] = the sites that show colour a
        in ladder 0's walker and colour b in ladder 1's walker at that slot
  launches: the sweeps (small route: 1 a round; HBM route: 2 swap_interval), + 3 when the round swaps or records (measure, final,
        swap pass), + 1 when it records (colour counts), + 1 when it records two ladders (tables)
The energies are fed in (the device's), as tempering_twin takes them, or come from potts_disorder_twin.energy, which restates the
device's summation order.  `fragile` decisions are counted: K12's site decisions as potts_disorder_twin defines them, and swap
decisions whose u lies within 1e-12 relative of exp(delta); the GPU tests run inputs that have none.
"""
import importlib.util
import math
import os

import numpy as np


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


pdt = _load("potts_disorder_twin")
tt = _load("tempering_twin")

SWAP_REL = 1e-12


def contingency(a, b, q):
    """C[a][b] of two colourings in Python integers: (q, q) int64, sum = sites."""
    C = [[0] * q for _ in range(q)]
    for x, y in zip(np.asarray(a).ravel().tolist(), np.asarray(b).ravel().tolist()):
        C[x][y] += 1
    return np.array(C, dtype=np.int64)


def overlap(C, q):
    """(q sum_a C[a][a] / N - 1) / (q - 1)."""
    C = np.asarray(C)
    return (q * np.trace(C, axis1=-2, axis2=-1) / C.sum(axis=(-2, -1)) - 1.0) / (q - 1.0)


def initial_colours(shape, q, seed, n_walkers, initial="random"):
    """The colours walker g starts from."""
    if initial == "random":
        return [np.random.default_rng(int(seed) + g).integers(0, q, size=shape).astype(np.int8) for g in range(n_walkers)]
    return [np.full(shape, int(initial), np.int8) for _ in range(n_walkers)]


def swap_fragile(walker_at_slot, T, E, u):
    """The decisions of one pass whose u lies within SWAP_REL (relative) of exp(delta), following the pass as it would go."""
    was = [int(w) for w in walker_at_slot]
    n = 0
    for i in range(len(was) - 1):
        a, b = was[i], was[i + 1]
        delta = (1.0 / float(T[i]) - 1.0 / float(T[i + 1])) * (float(E[a]) - float(E[b]))
        if delta < 0:
            x = math.exp(delta)
            if abs(float(u[i]) - x) <= SWAP_REL * x:
                n += 1
        if delta >= 0 or u[i] < np.exp(delta):
            was[i], was[i + 1] = b, a
    return n


class Ladders:
    """The whole state: spins[k][w], walker_at_slot (nl, R), flags, trips (nl, R), attempts / accepts (nl, R - 1), the counters, the
    launches and the fragile decisions met so far."""

    def __init__(self, shape, q, periodic, J, h, T, seed, ladders=1, initial="random", small=None, swap_rule=None):
        self.shape, self.q, self.periodic, self.J, self.h = tuple(shape), int(q), periodic, J, h
        self.T, self.seed, self.nl, self.R = [float(x) for x in T], int(seed), int(ladders), len(T)
        start = initial_colours(self.shape, self.q, self.seed, self.nl * self.R, initial)
        self.spins = [[start[k * self.R + w] for w in range(self.R)] for k in range(self.nl)]
        self.walker_at_slot = np.tile(np.arange(self.R), (self.nl, 1))
        self.flags = np.full((self.nl, self.R), tt.NONE)
        self.flags[:, 0] = tt.BOTTOM
        self.trips = np.zeros((self.nl, self.R), np.int64)
        self.attempts = np.zeros((self.nl, self.R - 1), np.int64)
        self.accepts = np.zeros((self.nl, self.R - 1), np.int64)
        self.sweeps = self.rounds = self.launches = self.fragile = 0
        self.small = int(np.prod(self.shape)) <= pdt.SMALL_SITES if small is None else bool(small)
        self.swap_rule = swap_rule or tt.swap_pass  # tests hand in a wrong rule to show they would see it

    def energy(self, k, w):
        return pdt.energy(self.spins[k][w], self.q, self.periodic, self.J, self.h)

    def energies(self):
        """(nl, R) by walker, in the device's summation order."""
        return np.array([[self.energy(k, w) for w in range(self.R)] for k in range(self.nl)])

    def run(self, n_rounds, interval, swap=True, record=True, energies=None):
        """energies(j, k) -> E by walker of ladder k in round j of this run (the device's); None: potts_disorder_twin.energy.
        Returns the recorded rows like PottsTemperingLattice.history()."""
        rows = {"E": [], "n_eq": [], "N": [], "walker": [], "tables": []}
        for j in range(n_rounds):
            for k in range(self.nl):
                for w in range(self.R):
                    T = self.T[int(np.flatnonzero(self.walker_at_slot[k] == w)[0])]
                    self.spins[k][w], f = pdt.sweep(self.spins[k][w], self.q, self.periodic, self.J, self.h, T, interval,
                                                    (self.seed + k * self.R + w) & (2 ** 64 - 1), self.sweeps & 0xFFFFFFFF, 0, with_fragile=True)
                    self.fragile += f
            self.sweeps += interval
            self.launches += 1 if self.small else 2 * interval
            if swap or record:
                Es = [np.asarray(energies(j, k)) if energies else np.array([self.energy(k, w) for w in range(self.R)])
                      for k in range(self.nl)]
                self.launches += 3
            if swap:
                for k in range(self.nl):
                    u = tt.swap_uniforms(self.R, self.rounds, self.seed, k)
                    self.fragile += swap_fragile(self.walker_at_slot[k], self.T, Es[k], u)
                    self.swap_rule(self.walker_at_slot[k], self.T, Es[k], u, self.attempts[k], self.accepts[k], self.flags[k], self.trips[k])
            if record:
                was = self.walker_at_slot.copy()
                meas = [[pdt.measure(self.spins[k][was[k, i]], self.q, self.periodic) for i in range(self.R)] for k in range(self.nl)]
                rows["walker"].append(was)
                rows["E"].append([[Es[k][was[k, i]] for i in range(self.R)] for k in range(self.nl)])
                rows["n_eq"].append([[int(m[0]) for m in lad] for lad in meas])
                rows["N"].append([[[int(v) for v in m[1][:self.q]] for m in lad] for lad in meas])
                self.launches += 1
                if self.nl == 2:
                    rows["tables"].append([contingency(self.spins[0][was[0, i]], self.spins[1][was[1, i]], self.q) for i in range(self.R)])
                    self.launches += 1
            self.rounds += 1
        n = n_rounds if record else 0
        return {"E": np.array(rows["E"], np.float64).reshape(n, self.nl, self.R),
                "n_eq": np.array(rows["n_eq"], np.int64).reshape(n, self.nl, self.R),
                "N": np.array(rows["N"], np.int64).reshape(n, self.nl, self.R, self.q),
                "walker": np.array(rows["walker"], np.int32).reshape(n, self.nl, self.R),
                "tables": np.array(rows["tables"], np.int64).reshape(n, self.R, self.q, self.q) if self.nl == 2 else None}


def inverted_swap_pass(walker_at_slot, T, E, u, attempts, accepts, flags, trips):
    """The reference's expression, E_b - E_a (gibbs.py:317): the inverse of the detailed-balance ratio.  Only for the test that shows
    the enumeration check sees it."""
    tt.swap_pass(walker_at_slot, T, -np.asarray(E, dtype=np.float64), u, attempts, accepts, flags, trips)


# ---------------------------------------------------------------- a tiny ladder in plain Python floats, for long chains
def tiny_chain(shape, q, periodic, J, h, T, seed, n_rounds, n_discard=0, inverted=False, block=2048):
    """One ladder of a lattice of at most 64 sites from colour 0 with one swap pass per sweep, in plain Python floats: (E by slot of
    every round after n_discard, (n_rounds - n_discard, R); fragile decisions; the statistics).  Bit for bit `Ladders(..., initial=0)`
    with run(n_rounds, 1), which tests/test_potts_pt_cpu.py asserts; it follows potts_disorder_twin.chain's per-site loop and
    potts_disorder_twin.energy's order so that 10^4 rounds take seconds, not hours."""
    shape3, per = pdt.lattice(shape, periodic)
    jr, jd, jl, hh = pdt.as_disorder(shape, periodic, J, h, q)
    n = int(np.prod(shape3))
    nbs = pdt._site_bonds(shape3, per, jr, jd, jl)
    h_of = [[0.0] * q for _ in range(n)] if hh is None else hh.astype(np.float64).reshape(q, n).T.tolist()
    col_of = pdt.p3.colours(shape3).ravel().tolist()
    of_colour = [[i for i in range(n) if col_of[i] == col] for col in (0, 1)]
    R = len(T)
    T = [float(t) for t in T]
    s = [[0] * n for _ in range(R)]
    was = list(range(R))
    att, acc = np.zeros(R - 1, np.int64), np.zeros(R - 1, np.int64)
    flags, trips = np.full(R, tt.NONE), np.zeros(R, np.int64)
    flags[0] = tt.BOTTOM
    out, n_fragile = [], 0

    assert n <= 64  # one wave: the energy below is potts_disorder_twin.energy's tree with its zero lanes left out
    D, Rr, C = shape3
    fwd = []  # per site: the bonds stored at it, in the order J_right, J_down, J_layer
    for z in range(D):
        for r in range(Rr):
            for c in range(C):
                fwd.append([(j, float(Jb[z, r, c])) for has, j, Jb in
                            (((c + 1 < C or per[2]), (z * Rr + r) * C + (c + 1) % C, jr), ((r + 1 < Rr or per[1]), (z * Rr + (r + 1) % Rr) * C + c, jd),
                             ((z + 1 < D or per[0]), (((z + 1) % D) * Rr + r) * C + c, jl)) if has])
    lanes = 1 << max(n - 1, 0).bit_length()

    def energy(sw):
        v = [0.0] * lanes
        for i in range(n):
            l = h_of[i][sw[i]]
            for j, Jb in fwd[i]:
                if sw[j] == sw[i]:
                    l += Jb
            v[i] = l
        off = lanes >> 1
        while off:
            for i in range(off):
                v[i] += v[i + off]
            off >>= 1
        return -v[0]

    done = 0
    while done < n_rounds:
        nb = min(block, n_rounds - done)
        U = [pdt.p3._uniform_block(shape3, done, nb, (int(seed) + w) & (2 ** 64 - 1), 0) for w in range(R)]
        for k in range(nb):
            slot_of = [0] * R
            for i, w in enumerate(was):
                slot_of[w] = i
            for w in range(R):
                Tw, sw = T[slot_of[w]], s[w]
                for col in (0, 1):
                    u_row = U[w][2 * k + col]
                    for i in of_colour[col]:
                        a = list(h_of[i])
                        for j, Jk in nbs[i]:
                            a[sw[j]] += Jk
                        amax = max(a)
                        Z, accw = [], 0.0
                        for c in range(q):
                            wgt = math.exp((a[c] - amax) / Tw)
                            accw = wgt if c == 0 else accw + wgt
                            Z.append(accw)
                        u = u_row[i]
                        new = q - 1
                        for c in range(q - 2, -1, -1):
                            real = Z[c] / accw * pdt.TWO32
                            if abs(u - real) <= 1.0:
                                n_fragile += 1
                            if u < math.floor(real + 0.5):
                                new = c
                        sw[i] = new
            E = [energy(s[w]) for w in range(R)]
            us = tt.swap_uniforms(R, done + k, seed, 0)
            n_fragile += swap_fragile(was, T, [-e for e in E] if inverted else E, us)
            (inverted_swap_pass if inverted else tt.swap_pass)(was, T, E, us, att, acc, flags, trips)
            if done + k >= n_discard:
                out.append([E[w] for w in was])
        done += nb
    return np.array(out), n_fragile, {"attempts": att, "accepts": acc, "round_trips": trips, "walker_at_slot": np.array(was)}


def exact_energies(shape, q, periodic, J, h, temperatures):
    """<E> at every temperature by enumeration of the q^N states."""
    shape3, per = pdt.lattice(shape, periodic)
    jr, jd, jl, hh = pdt.as_disorder(shape, periodic, J, h, q)
    n_sites = int(np.prod(shape3))
    n_states = int(q) ** n_sites
    E = np.zeros(n_states)
    chunk = 1 << 16
    for lo in range(0, n_states, chunk):
        k = np.arange(lo, min(lo + chunk, n_states), dtype=np.int64)
        digits = np.stack([(k // int(q) ** i) % int(q) for i in range(n_sites)], axis=1).reshape((k.size,) + shape3)
        e = np.zeros(k.size)
        for axis, Jb in ((2, jr), (1, jd), (0, jl)):
            Jm = Jb.astype(np.float64).copy()
            if not per[axis]:
                edge = [slice(None)] * 3
                edge[axis] = -1
                Jm[tuple(edge)] = 0.0
            e -= ((digits == np.roll(digits, -1, axis + 1)) * Jm[None]).sum(axis=(1, 2, 3))
        if hh is not None:
            e -= np.take_along_axis(np.broadcast_to(hh.astype(np.float64)[None], (k.size,) + hh.shape), digits[:, None], axis=1)[:, 0].sum(axis=(1, 2, 3))
        E[lo:lo + k.size] = e
    out = []
    for T in temperatures:
        w = np.exp(-(E - E.min()) / float(T))
        out.append(float((E * w).sum() / w.sum()))
    return np.array(out)


def batch_means_error(x, n_batches=32):
    """The batch-means standard error of the mean of a series."""
    x = np.asarray(x, dtype=np.float64)
    m = x[:x.size // n_batches * n_batches].reshape(n_batches, -1).mean(axis=1)
    return float(m.std(ddof=1) / math.sqrt(n_batches))


# ---------------------------------------------------------------- the cases of tests/test_potts_pt_gpu.py
# Every bit-for-bit GPU case is listed here so that tests/test_potts_pt_cpu.py can assert, without a device, that none holds a fragile
# decision.  4 rounds of 3 sweeps with swaps.
N_ROUNDS, INTERVAL = 4, 3
SHAPES = [((5, 19), False), ((6, 32), True), ((3, 4, 18), (False, True, True)), ((4, 4, 16), True)]


def cases():
    """shape x q, cycling field, R and ladders so that each occurs with each shape; the (6, 32) q = 3 case starts with its sweep
    counter at 2^32 - 5, so that the counter's word wraps inside the run."""
    out = []
    for i, (shape, per) in enumerate(SHAPES):
        for j, q in enumerate((2, 3, 8)):
            k = len(out)
            out.append(dict(shape=shape, periodic=per, q=q, field=bool((i + j) % 2), R=(2, 5)[(i + j // 2 + j) % 2], ladders=(1, 2)[(k // 2 + i) % 2],
                            seed=pdt.SEEDS[k % 3] - (16 if k % 3 == 0 else 0), dseed=300 + k, sweep0=2 ** 32 - 5 if (i, q) == (1, 3) else 0))
    return out


def case_id(c):
    per = c["periodic"]
    tag = "p" if per is True else ("o" if per is False else "".join("po"[not x] for x in per))
    return "x".join(map(str, c["shape"])) + f"-{tag}-q{c['q']}" + ("-h" if c["field"] else "") + f"-R{c['R']}-L{c['ladders']}" + ("-wrap" if c["sweep0"] else "")


def case_temperatures(R):
    return np.linspace(0.6, 2.4, R)


def case_disorder(c):
    return pdt.random_disorder(c["shape"], c["periodic"], c["q"], np.random.default_rng(c["dseed"]), "gaussian", c["field"])


def case_twin(c, small=None):
    J, h = case_disorder(c)
    lad = Ladders(c["shape"], c["q"], c["periodic"], J, h, case_temperatures(c["R"]), c["seed"], c["ladders"], small=small)
    lad.sweeps = c["sweep0"]
    return lad


# the long ladder, the route boundary and the enumeration case of the GPU file
LONG = dict(shape=(4, 16), periodic=True, q=3, field=True, R=130, ladders=2, seed=777, dseed=350, sweep0=0)
LONG_ROUNDS, LONG_INTERVAL = 3, 1
BOUNDARY = [dict(shape=(128, 128), periodic=True, q=3, field=False, R=2, ladders=1, seed=31, dseed=360, sweep0=0),
            dict(shape=(128, 130), periodic=True, q=3, field=False, R=2, ladders=1, seed=32, dseed=361, sweep0=0)]
# open 3 x 4, q = 3, Gaussian couplings and site field, 4 temperatures, one swap pass per sweep
ENUM = dict(shape=(3, 4), periodic=False, q=3, T=(0.5, 0.8, 1.3, 2.0), dseed=21, seed=9000, n_discard=500, n_rounds=20500)


def enum_disorder():
    return pdt.random_disorder(ENUM["shape"], ENUM["periodic"], ENUM["q"], np.random.default_rng(ENUM["dseed"]), "gaussian", True)

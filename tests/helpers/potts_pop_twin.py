"""NumPy / Python-integer twin of K14, population annealing of K12's Potts lattice (tsu_potts_pop_*, csrc/potts_pop.hip).

Contract ("Population annealing of Potts lattices (K14)"), R walkers on one disorder, beta[0] < .. < beta[K]:
  walker i: a K12 lattice (potts_disorder_twin) with key seed + i, replica 0 and the shared 32-bit sweep counter
  draw: site (rho, c) of walker i = ((uint64) W q) >> 32, W = word c & 3 of Philox(c >> 2, rho, 0, TAG_INIT = 2), key seed + i
  step k: population_twin's weights, offset, counts and placement (the step of tsu_hip_population.h), the colours parent[i] -> i, then
        sweeps_per_step potts_disorder_twin sweeps of every walker at T = 1.0 / beta[k], then E, n_eq and N_c of every walker
  launches: a step on _PACK / _SMALL 1 (0 without sweeps) + 2 (+ 2 when it resamples); on _SWEEP 2 sweeps_per_step + 2 (+ 2)
This file composes population_twin (the resampler, check_step) with potts_disorder_twin (sweep, measure, energy, fragile decisions)
and adds the draw, the mirror of the packing rule (csrc/potts_pop_plan.h), exact ln Z and <E> by enumeration, a plain vectorised
population annealing with NumPy's generator (the statistical reference of the enumeration criterion) and the case tables of
tests/test_potts_pop_gpu.py.
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
pop = _load("population_twin")

TAG_INIT = 2
MASK64 = 2 ** 64 - 1


# ---------------------------------------------------------------- the device draw
def draw_colour(W, q):
    """potts_pop_draw: ((uint64) W q) >> 32."""
    return (int(W) * int(q)) >> 32


def draw(shape, q, seed, n_walkers):
    """(n_walkers,) + shape int8: the colours init(seed, -2) gives every walker."""
    shape3, _ = pdt.lattice(shape, True if len(shape) == 3 else False)
    D, R, C = shape3
    keys = [(int(seed) + i) & MASK64 for i in range(n_walkers)]
    k0 = np.array([k & 0xFFFFFFFF for k in keys], np.uint64)[:, None, None]
    k1 = np.array([k >> 32 for k in keys], np.uint64)[:, None, None]
    rho = np.arange(D * R, dtype=np.uint64)[None, :, None]
    quad = np.arange((C + 3) >> 2, dtype=np.uint64)[None, None, :]
    W = np.stack(pop.philox(quad, rho, 0, TAG_INIT, k0, k1))  # (4, n_walkers, D R, quads)
    c = np.arange(C)
    words = W[c & 3, :, :, c >> 2]  # (C, n_walkers, D R)
    col = (words.astype(np.uint64) * np.uint64(q)) >> np.uint64(32)
    return np.moveaxis(col, 0, -1).astype(np.int8).reshape((n_walkers,) + tuple(shape))


# ---------------------------------------------------------------- the packing rule (csrc/potts_pop_plan.h)
ROUTES = ("k14_pop_pack", "k14_pop_small", "k14_pop_sweep")
PACK_THREADS, PACK_MAX_LANES, PACK_LDS, SMALL_SITES, SMALL_MAX_THREADS = 256, 128, 64 * 1024, 16384, 1024


def lanes(shape):
    return int(np.prod(shape[:-1])) * ((shape[-1] + 15) >> 4)


def stride(sites):
    return (sites + 15) // 16 * 16


def plan(sites, n_lanes, dim, q, has_field, R, allow_pack=True, allow_small=True):
    """(route index, G, threads, lds_bytes) as potts_pop_plan gives them."""
    if not allow_small or sites > SMALL_SITES:
        return (2, 1, 256, 0)
    small = (1, 1, min((n_lanes + 63) // 64 * 64, SMALL_MAX_THREADS), SMALL_SITES)
    if not allow_pack or n_lanes > PACK_MAX_LANES:
        return small
    G = min(PACK_THREADS // n_lanes, R)
    lds = 4 * ((2 if dim == 2 else 3) + (q if has_field else 0)) * sites + G * stride(sites)
    if G < 2 or lds > PACK_LDS:
        return small
    return (0, G, (G * n_lanes + 63) // 64 * 64, lds)


def plan_of(shape, periodic, q, has_field, R, **kw):
    shape3, per = pdt.lattice(shape, periodic)
    dim = 2 if shape3[0] == 1 and not per[0] else 3
    r, G, t, b = plan(int(np.prod(shape)), lanes(shape3), dim, q, has_field, R, **kw)
    return {"route": ROUTES[r], "G": G, "threads": t, "lds_bytes": b}


def step_launches(route, sweeps_per_step, resample):
    sweeps = 2 * sweeps_per_step if route == "k14_pop_sweep" else (1 if sweeps_per_step else 0)
    return sweeps + 2 + (2 if resample else 0)


# ---------------------------------------------------------------- the population
class Population:
    """The whole state: spins (R,) + shape, E, the counters and the fragile decisions met so far.  `walkers`: the indices that are
    swept and measured (None: all); the others keep their colours (for the tests without resampling, which compare a few walkers)."""

    def __init__(self, shape, q, periodic, J, h, betas, seed, R, initial="random", initial_sweeps=0, sweep0=0, walkers=None):
        self.shape, self.q, self.periodic, self.J, self.h = tuple(shape), int(q), periodic, J, h
        self.betas, self.seed, self.R = [float(b) for b in betas], int(seed), int(R)
        self.spins = draw(self.shape, self.q, self.seed, self.R) if initial == "random" else np.full((self.R,) + self.shape, int(initial), np.int8)
        self.walkers = list(range(self.R)) if walkers is None else list(walkers)
        self.sweeps, self.offset, self.step, self.fragile = 0, 0, 0, 0
        if self.betas[0] > 0:
            self._sweep(1.0 / self.betas[0], initial_sweeps)
        self.offset = int(sweep0)  # init starts the counter at 0; advance(sweep0) follows it

    def _sweep(self, T, n):
        for i in self.walkers:
            self.spins[i], f = pdt.sweep(self.spins[i], self.q, self.periodic, self.J, self.h, T, n, (self.seed + i) & MASK64,
                                         (self.offset + self.sweeps) & 0xFFFFFFFF, 0, with_fragile=True)
            self.fragile += f
        self.sweeps += n

    def energies(self):
        return np.array([pdt.energy(self.spins[i], self.q, self.periodic, self.J, self.h) for i in self.walkers])

    def measure(self):
        m = [pdt.measure(self.spins[i], self.q, self.periodic) for i in self.walkers]
        return np.array([int(x[0]) for x in m], np.int64), np.array([[int(v) for v in x[1][:self.q]] for x in m], np.int64)

    def run(self, n_steps, sweeps_per_step, resample=True, energies=None):
        """energies(j) -> the device's E of every walker before step j of this run (None: potts_disorder_twin.energy).  Returns the
        rows like PottsPopulation.history() for the walkers it follows."""
        rows = {k: [] for k in ("E", "n_eq", "N", "W", "parent", "S", "U", "E_min")}
        E = self.energies()
        n_eq, N = self.measure()
        for k in ("E", "n_eq", "N"):
            rows[k].append({"E": E, "n_eq": n_eq, "N": N}[k])
        for j in range(n_steps):
            k = self.step + 1
            if resample:
                assert len(self.walkers) == self.R
                Ein = np.asarray(energies(j)) if energies else E
                W, e_min = pop.weights(Ein, self.betas[k] - self.betas[k - 1])
                res = pop.resample(W, self.step, self.seed)
                self.spins = self.spins[np.asarray(res["parent"])]
                for key, v in (("W", W), ("parent", res["parent"]), ("S", res["S"]), ("U", res["U"]), ("E_min", e_min)):
                    rows[key].append(v)
            else:
                for key, v in (("W", [0] * self.R), ("parent", list(range(self.R))), ("S", 0), ("U", 0), ("E_min", 0.0)):
                    rows[key].append(v)
            self._sweep(1.0 / self.betas[k], sweeps_per_step)
            E = self.energies()
            n_eq, N = self.measure()
            rows["E"].append(E)
            rows["n_eq"].append(n_eq)
            rows["N"].append(N)
            self.step += 1
        return {"E": np.array(rows["E"]), "n_eq": np.array(rows["n_eq"]), "N": np.array(rows["N"]),
                "W": np.array(rows["W"], np.uint32).reshape(n_steps, self.R), "parent": np.array(rows["parent"], np.int32).reshape(n_steps, self.R),
                "S": np.array(rows["S"], np.uint64), "U": np.array(rows["U"], np.uint64), "E_min": np.array(rows["E_min"], np.float64)}


def free_energy(betas, S, E_min, mean_E, R, n_sites, q):
    """ln_Z, F, entropy as tsu.models.potts_population.potts_population_free_energy gives them, in plain Python floats."""
    ln_Z = [n_sites * math.log(q) if betas[0] == 0 else 0.0]
    for j in range(len(S)):
        ln_Z.append(ln_Z[-1] + (-(betas[j + 1] - betas[j]) * float(E_min[j]) + math.log(float(S[j]) / (R * float(pop.ONE)))))
    return np.array(ln_Z)


# ---------------------------------------------------------------- exact values by enumeration
def state_energies(shape, q, periodic, J, h):
    """E of all q^N states, state k's site i showing digit i of k in base q (row-major sites)."""
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
            hb = np.broadcast_to(hh.astype(np.float64)[None], (k.size,) + hh.shape)
            e -= np.take_along_axis(hb, digits[:, None], axis=1)[:, 0].sum(axis=(1, 2, 3))
        E[lo:lo + k.size] = e
    return E


def exact(E_states, betas):
    """(ln Z, <E>) at every beta from the energies of all states."""
    e0 = E_states.min()
    lnZ, mE = [], []
    for b in betas:
        w = np.exp(-float(b) * (E_states - e0))
        lnZ.append(math.log(w.sum()) - float(b) * e0)
        mE.append(float((E_states * w).sum() / w.sum()))
    return np.array(lnZ), np.array(mE)


# ---------------------------------------------------------------- the statistical reference: plain population annealing in NumPy
def reference_anneal(shape, q, periodic, J, h, betas, R, sweeps_per_step, rng, resample=True):
    """(ln_Z, <E>) per beta of one population-annealing run with NumPy's generator: uniform start, systematic resampling with real
    weights, checkerboard heat-bath sweeps of all walkers at once.  Not bit-compatible with the device; the same algorithm."""
    shape3, per = pdt.lattice(shape, periodic)
    jr, jd, jl, hh = pdt.as_disorder(shape, periodic, J, h, q)
    Js = {0: jl.astype(np.float64), 1: jd.astype(np.float64), 2: jr.astype(np.float64)}
    for axis in range(3):
        if not per[axis]:
            edge = [slice(None)] * 3
            edge[axis] = -1
            Js[axis][tuple(edge)] = 0.0
    hq = np.zeros((q,) + shape3) if hh is None else hh.astype(np.float64)
    n = int(np.prod(shape3))
    idx = np.indices(shape3)
    parity = (idx[0] + idx[1] + idx[2]) & 1
    s = rng.integers(0, q, size=(R,) + shape3)

    def sums(s):  # (R, q, D, Rr, C): a_c of every site
        a = np.broadcast_to(hq[None], (R,) + hq.shape).copy()
        for axis in range(3):
            fw, bw = np.roll(s, -1, axis + 1), np.roll(s, 1, axis + 1)
            Jb = np.roll(Js[axis], 1, axis)
            for c in range(q):
                a[:, c] += (fw == c) * Js[axis][None] + (bw == c) * Jb[None]
        return a

    def energy(s):
        e = -np.take_along_axis(np.broadcast_to(hq[None], (R,) + hq.shape), s[:, None], axis=1)[:, 0].sum(axis=(1, 2, 3))
        for axis in range(3):
            e -= ((s == np.roll(s, -1, axis + 1)) * Js[axis][None]).sum(axis=(1, 2, 3))
        return e

    E = energy(s)
    lnZ, mE = [n * math.log(q) if betas[0] == 0 else 0.0], [E.mean()]
    for k in range(1, len(betas)):
        db = betas[k] - betas[k - 1]
        if resample:
            w = np.exp(-db * (E - E.min()))
            lnZ.append(lnZ[-1] - db * E.min() + math.log(w.mean()))
            C = np.cumsum(w) / w.sum() * R
            u = rng.random()
            cnt = np.floor(C + u).astype(np.int64)
            cnt = np.diff(np.concatenate([[0], cnt]))
            cnt[-1] += R - cnt.sum()
            s = np.repeat(s, cnt, axis=0)
        else:
            lnZ.append(np.nan)
        for _ in range(sweeps_per_step):
            for colour in (0, 1):
                a = sums(s)
                p = np.exp(betas[k] * (a - a.max(axis=1, keepdims=True)))
                cum = np.cumsum(p, axis=1)
                u = rng.random((R, 1) + shape3) * cum[:, -1:]
                new = (u >= cum).sum(axis=1)
                s = np.where((parity == colour)[None], np.minimum(new, q - 1), s)
        E = energy(s)
        mE.append(E.mean())
    return np.array(lnZ), np.array(mE)


def criterion(lnZ_runs, E_runs, lnZ_exact, E_exact):
    """The worst |mean - exact| / (spread over the M runs / sqrt(M)) over ln Z (beta > beta[0]) and <E> (every beta)."""
    lnZ_runs, E_runs = np.asarray(lnZ_runs), np.asarray(E_runs)
    M = lnZ_runs.shape[0]
    worst = 0.0
    for runs, ex, lo in ((lnZ_runs, lnZ_exact, 1), (E_runs, E_exact, 0)):
        err = runs[:, lo:].std(axis=0, ddof=1) / math.sqrt(M)
        worst = max(worst, float(np.max(np.abs(runs[:, lo:].mean(axis=0) - ex[lo:]) / err)))
    return worst


# ---------------------------------------------------------------- the cases of tests/test_potts_pop_gpu.py
# Every bit-for-bit GPU case is listed here so that tests/test_potts_pop_cpu.py can assert, without a device, that the walkers it
# compares hold no fragile decision.
R_SINGLE = 70
SHAPES = [((6, 32), True), ((5, 37), False), ((16, 16), True), ((3, 4, 18), (False, True, True))]
SCHEDULES = [dict(betas=[0.0, 0.3, 0.7, 1.2], initial_sweeps=0), dict(betas=[0.4, 0.9, 1.5, 1.6], initial_sweeps=3)]
SWEEPS_PER_STEP = 2


def single_cases():
    """Every shape with every q and both fields; the schedules alternate, and the (6, 32) q = 3 cases start their sweep counter at
    2^32 - 4, so that the counter's word wraps inside the run."""
    out = []
    for i, (shape, per) in enumerate(SHAPES):
        for j, q in enumerate((2, 3, 8)):
            for field in (False, True):
                k = len(out)
                out.append(dict(shape=shape, periodic=per, q=q, field=field, schedule=(i + j + int(field)) % 2, seed=pdt.SEEDS[k % 3] - (80 if k % 3 == 0 else 0),
                                dseed=400 + k, sweep0=2 ** 32 - 4 if (i, q) == (0, 3) else 0))
    return out


def case_id(c):
    per = c["periodic"]
    tag = "p" if per is True else ("o" if per is False else "".join("po"[not x] for x in per))
    return "x".join(map(str, c["shape"])) + f"-{tag}-q{c['q']}" + ("-h" if c["field"] else "") + f"-s{c['schedule']}" + ("-wrap" if c["sweep0"] else "")


def case_disorder(c):
    return pdt.random_disorder(c["shape"], c["periodic"], c["q"], np.random.default_rng(c["dseed"]), "gaussian", c["field"])


def single_walkers(c):
    """The walkers the single-model test compares: 0, G - 1, G and R - 1 of the shipped plan (G = 1 off _PACK: 0, 1, R - 1)."""
    G = plan_of(c["shape"], c["periodic"], c["q"], c["field"], R_SINGLE)["G"]
    return sorted({0, max(G - 1, 0), G, R_SINGLE - 1})


def single_twin(c):
    J, h = case_disorder(c)
    sch = SCHEDULES[c["schedule"]]
    return Population(c["shape"], c["q"], c["periodic"], J, h, sch["betas"], c["seed"], R_SINGLE, initial_sweeps=sch["initial_sweeps"],
                      sweep0=c["sweep0"], walkers=single_walkers(c))


# the resampled chains: 4 x 4 and 3 x 4 (12 sites: the stride is padded), R and the step width
CHAIN_CASES = [dict(shape=shape, periodic=per, q=q, field=field, R=R, db=db, seed=5000 + 17 * k, dseed=450 + k)
               for k, (shape, per, q, field, R, db) in enumerate([
                   ((4, 4), True, 3, True, 3, 0.3), ((3, 4), False, 3, True, 65, 1e-9), ((4, 4), True, 2, False, 65, 5.0),
                   ((3, 4), False, 8, False, 1025, 0.3), ((3, 4), False, 2, True, 3, 5.0), ((4, 4), True, 8, True, 1025, 1e-9)])]
CHAIN_STEPS, CHAIN_SWEEPS = 3, 2


def chain_betas(c):
    return [0.2 + c["db"] * k for k in range(CHAIN_STEPS + 1)]


# the enumeration cases: (shape, q, periodic, field, dseed); beta 0 .. 1.5 in 30 steps, 5 sweeps a step, M seeds of R walkers
ENUM_CASES = [((3, 4), 3, False, True, 21), ((2, 2, 3), 2, False, True, 22)]
ENUM_BETAS = np.linspace(0.0, 1.5, 31)
ENUM_SWEEPS, ENUM_R, ENUM_M, ENUM_SIGMAS = 5, 1024, 32, 4.0


def enum_disorder(case):
    shape, q, per, field, dseed = case
    return pdt.random_disorder(shape, per, q, np.random.default_rng(dseed), "gaussian", field)

"""Multicanonical (flat-histogram) sampling of q-state Potts lattices (K11): thousands of independent walkers that share one weight
table ln W[n_eq] and add to one exact histogram, the sampler for the first-order transitions (q >= 5 in 2-D, q >= 3 in 3-D) where
every canonical method of this package tunnels exponentially slowly.

The walkers sample W(n_eq) in place of exp(-E / T), n_eq the number of satisfied bonds and E = -J n_eq; the weight recursion, the
density of states and the reweighting to a temperature are float64 arithmetic on the host (:func:`muca_recursion`,
:func:`muca_density_of_states`, :func:`muca_reweight`, which need no GPU); every sweep runs in ``csrc/potts_muca.hip``.  The reference has
no counterpart; the method is Berg and Neuhaus's, the parallel form Gross, Zierenberg, Weigel and Janke's (CPC 2018).
"""
import math

import numpy as np

from .. import _hip
from ..core import ConfigurationError


def _logsumexp(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max()
    return m + math.log(np.exp(x - m).sum())


MUCA_EDGE_BINS = 16     # visited bins at each end of the range whose least-squares slope continues ln W beyond it
MUCA_EDGE_SLOPE = 4.0   # and the largest |slope| per level taken from them


def muca_recursion(lnw, H):
    """One weight iteration: ln W[n] -= ln H[n] on the visited bins; the bins outside the visited range are continued *linearly*
    from its ends, with the least-squares slope of the new ln W over the outermost ``MUCA_EDGE_BINS`` visited bins (at most
    ``MUCA_EDGE_SLOPE`` per level), so that the walkers are drawn on into the steep ends of ln g, where a flat continuation leaves
    them climbing the entropy unaided; unvisited bins inside the range are left alone; the maximum is shifted to 0."""
    lnw = np.array(lnw, dtype=np.float64)
    H = np.asarray(H, dtype=np.float64)
    seen = np.flatnonzero(H > 0)
    if seen.size == 0:
        return lnw
    lo, hi = int(seen[0]), int(seen[-1])
    lnw[seen] -= np.log(H[seen])
    n = np.arange(lnw.size, dtype=np.float64)
    for edge, outside, anchor in ((seen[:MUCA_EDGE_BINS], n < lo, lo), (seen[-MUCA_EDGE_BINS:], n > hi, hi)):
        slope = float(np.polyfit(edge.astype(np.float64), lnw[edge], 1)[0]) if edge.size >= 2 else 0.0
        slope = min(max(slope, -MUCA_EDGE_SLOPE), MUCA_EDGE_SLOPE)
        lnw[outside] = lnw[anchor] + slope * (n[outside] - anchor)
    return lnw - lnw.max()


def muca_flatness(H):
    """(n_lo, n_hi, flatness, holes) of a histogram: the visited range, min / mean of H over the visited bins of it, and the number
    of bins inside it that hold no entry (levels without a state, such as B - 1 on a periodic lattice, or levels not reached yet).
    (0, -1, 0.0, 0) for an empty record."""
    H = np.asarray(H, dtype=np.float64)
    seen = np.flatnonzero(H > 0)
    if seen.size == 0:
        return 0, -1, 0.0, 0
    lo, hi = int(seen[0]), int(seen[-1])
    return lo, hi, float(H[seen].min() / H[seen].mean()), hi - lo + 1 - int(seen.size)


def muca_density_of_states(H, lnw, q, n_sites):
    """ln g[n] = ln H[n] - ln W[n] on the visited bins (-inf elsewhere), normalised to sum g = q^N by log-sum-exp."""
    H = np.asarray(H, dtype=np.float64)
    lnw = np.asarray(lnw, dtype=np.float64)
    seen = H > 0
    if not seen.any():
        raise ValueError("the record is empty")
    ln_g = np.full(H.shape, -np.inf)
    ln_g[seen] = np.log(H[seen]) - lnw[seen]
    return ln_g + (n_sites * math.log(q) - _logsumexp(ln_g[seen]))


def muca_reweight(H, S1, S2, lnw, temperatures, coupling, q, n_sites):
    """The canonical averages at each temperature from a multicanonical record: level n carries H[n] / W[n] exp(J n / T), all by
    log-sum-exp.  Returns arrays over the temperatures: ``energy`` (per site, -J <n_eq> / N), ``specific_heat`` = N var(e) / T^2,
    ``order_parameter`` = (q <N_max> / N - 1) / (q - 1) (``potts_order_parameter``'s convention), ``susceptibility`` =
    N var(m) / T, and the plain averages ``n_eq``, ``n_max`` and ``n_max2`` (<N_max^2>) they are made of.  ``coupling`` of either
    sign."""
    H, S1, S2 = (np.asarray(a, dtype=np.float64) for a in (H, S1, S2))
    lnw = np.asarray(lnw, dtype=np.float64)
    seen = np.flatnonzero(H > 0)
    if seen.size == 0:
        raise ValueError("the record is empty")
    n = seen.astype(np.float64)
    base = np.log(H[seen]) - lnw[seen]
    m1, m2 = S1[seen] / H[seen], S2[seen] / H[seen]
    J, N = float(coupling), float(n_sites)
    out = {k: [] for k in ("energy", "specific_heat", "order_parameter", "susceptibility", "n_eq", "n_max", "n_max2")}
    for T in (float(t) for t in temperatures):
        if not (math.isfinite(T) and T > 0):
            raise ValueError("Temperature must be positive")
        lp = base + J * n / T
        p = np.exp(lp - _logsumexp(lp))
        n1, n2 = float(p @ n), float(p @ (n * n))
        a1, a2 = float(p @ m1), float(p @ m2)
        scale = q / (N * (q - 1.0))
        out["n_eq"].append(n1)
        out["n_max"].append(a1)
        out["n_max2"].append(a2)
        out["energy"].append(-J * n1 / N)
        out["specific_heat"].append(J * J * max(n2 - n1 * n1, 0.0) / (N * T * T))
        out["order_parameter"].append((q * a1 / N - 1.0) / (q - 1.0))
        out["susceptibility"].append(N * scale * scale * max(a2 - a1 * a1, 0.0) / T)
    res = {k: np.array(v) for k, v in out.items()}
    res["temperatures"] = np.array([float(t) for t in temperatures])
    return res


def check_muca_model(size, q, walkers, coupling, periodic):
    """The refusals, made on the host before the device is touched; returns ((D, R, C), (p_z, p_r, p_c), the user's lattice shape).
    A 2-D size is one layer with an open depth axis."""
    if isinstance(q, bool) or int(q) != q or not 2 <= int(q) <= _hip.POTTS_MAX_Q:
        raise ConfigurationError(f"q must be an integer in 2 .. {_hip.POTTS_MAX_Q} (got {q!r})")
    try:
        user = (int(size),) * 2 if np.isscalar(size) else tuple(int(v) for v in size)
    except (TypeError, ValueError):
        raise ConfigurationError("size must be an int, (rows, cols) or (depth, rows, cols)") from None
    if len(user) not in (2, 3) or min(user) < 1:
        raise ConfigurationError("size must be a positive int, (rows, cols) or (depth, rows, cols)")
    try:
        if isinstance(periodic, (bool, np.bool_)):
            per = (bool(periodic),) * 3 if len(user) == 3 else (False, bool(periodic), bool(periodic))
        else:
            per = tuple(bool(x) for x in periodic)
            if len(per) != len(user):
                raise ValueError
            per = per if len(user) == 3 else (False,) + per
    except (TypeError, ValueError):
        raise ConfigurationError("periodic must be a bool or one flag per axis of size") from None
    shape = user if len(user) == 3 else (1,) + user
    sites = shape[0] * shape[1] * shape[2]
    if sites > _hip.POTTS_MUCA_MAX_SITES:
        raise ConfigurationError(f"the lattice must hold at most {_hip.POTTS_MUCA_MAX_SITES} sites")
    if isinstance(walkers, bool) or int(walkers) != walkers or not 1 <= int(walkers) <= _hip.POTTS_MUCA_MAX_WALKERS:
        raise ConfigurationError(f"walkers must be an integer in 1 .. {_hip.POTTS_MUCA_MAX_WALKERS}")
    if int(walkers) * sites > 2 ** 31 - 1:
        raise ConfigurationError("walkers * sites must not exceed 2^31 - 1")
    if not math.isfinite(float(coupling)):
        raise ConfigurationError("coupling must be finite")
    return shape, per, user


class PottsMulticanonical:
    """``walkers`` independent copies of a q-state Potts lattice under one multicanonical weight table, on the GPU between calls.

    ``size``: an int (L x L), (R, C) or (D, R, C); ``periodic``: a bool or one flag per axis; any side >= 1, odd periodic sides
    included.  The walkers start with every colour 0 and ln W = 0.  ``run(n)`` sweeps every walker n times with the current weights
    and adds to the record; ``iterate(n)`` is one step of the weight recursion; ``density_of_states()`` and ``reweight(T)`` turn
    the record into physics.  ``coupling`` (either sign) enters only there.  ``weights`` is ln W[0 .. B] over n_eq.
    """

    def __init__(self, size, q, walkers, coupling: float = 1.0, periodic=True, seed: int = 0):
        self._shape3, self.periodic, self.shape = check_muca_model(size, q, walkers, coupling, periodic)
        self.q, self.walkers, self.coupling = int(q), int(walkers), float(coupling)
        self.seed = _hip._seed(seed)
        self.n_spins = self._shape3[0] * self._shape3[1] * self._shape3[2]
        self.sweep_count = 0
        self._h = _hip.PottsMucaWalkers(*self._shape3, self.q, self.walkers, self.periodic)
        self.bonds, self.z_max = self._h.bonds, self._h.z_max
        self._lnw = np.zeros(self.bonds + 1)
        self._tunnels_seen = 0

    def close(self) -> None:
        self._h.close()

    @property
    def weights(self) -> np.ndarray:
        return self._lnw.copy()

    @weights.setter
    def weights(self, lnw) -> None:
        w = np.array(lnw, dtype=np.float64)
        if w.shape != (self.bonds + 1,) or not np.all(np.isfinite(w)):
            raise ValueError(f"weights must hold B + 1 = {self.bonds + 1} finite values")
        self._h.set_weights(w)
        self._lnw = w

    @property
    def spins(self) -> np.ndarray:
        return self._h.get_spins().reshape((self.walkers,) + self.shape)

    @spins.setter
    def spins(self, colours) -> None:
        s = np.asarray(colours)
        if s.shape != (self.walkers,) + self.shape:
            raise ValueError(f"spins must have shape {(self.walkers,) + self.shape}")
        if not np.issubdtype(s.dtype, np.integer) or s.min() < 0 or s.max() >= self.q:
            raise ValueError(f"spins must be integer colours in 0 .. {self.q - 1}")
        self._h.set_spins(s.astype(np.int8))

    def fill(self, colour: int):
        if not 0 <= int(colour) < self.q:
            raise ValueError(f"colour must be in 0 .. {self.q - 1}")
        self._h.fill(int(colour))
        return self

    def run(self, n_sweeps: int):
        self._h.run(int(n_sweeps), self.seed, self.sweep_count & 0xFFFFFFFF)
        self.sweep_count += int(n_sweeps)
        return self

    def histogram(self) -> np.ndarray:
        return self._h.record()[0]

    def moments(self):
        """(S1, S2): the sums of N_max and of N_max^2 per level, exact integers."""
        _, s1, s2 = self._h.record()
        return s1, s2

    def clear_record(self):
        self._h.clear_record()
        return self

    def energies(self) -> np.ndarray:
        """n_eq of every walker (the energy is -coupling n_eq)."""
        return self._h.energies()

    def tunnels(self) -> np.ndarray:
        return self._h.tunnels()

    def set_tunnel_bounds(self, n_lo: int, n_hi: int):
        """A walker tunnels when it goes from n_eq <= n_lo to n_eq >= n_hi or back (default (0, B)); clears the counts."""
        if not 0 <= int(n_lo) < int(n_hi) <= max(self.bonds, 1):
            raise ValueError("need 0 <= n_lo < n_hi <= B")
        self._h.set_tunnel_bounds(int(n_lo), int(n_hi))
        self._tunnels_seen = 0
        return self

    def consistent(self) -> bool:
        """Recount n_eq and the colour counts of every walker from the spins on the device; True iff the kept ones agreed."""
        return self._h.measure()

    def route(self) -> str:
        return self._h.route()

    def launch_count(self) -> int:
        return self._h.launch_count()

    def iterate(self, n_sweeps: int) -> dict:
        """Clear the record, run ``n_sweeps`` sweeps, then one step of :func:`muca_recursion`.  Returns ``range`` (the visited
        n_lo, n_hi), ``flatness`` (min / mean of H over its visited bins), ``holes`` (its bins without an entry) and ``tunnel_events``
        (of all walkers, during this call)."""
        self.clear_record()
        self.run(n_sweeps)
        H = self.histogram()
        lo, hi, flat, holes = muca_flatness(H)
        total = int(self.tunnels().sum(dtype=np.int64))
        events, self._tunnels_seen = total - self._tunnels_seen, total
        self.weights = muca_recursion(self._lnw, H)
        return {"range": (lo, hi), "flatness": flat, "holes": holes, "tunnel_events": events}

    def density_of_states(self) -> np.ndarray:
        return muca_density_of_states(self.histogram(), self._lnw, self.q, self.n_spins)

    def reweight(self, temperatures) -> dict:
        H, s1, s2 = self._h.record()
        return muca_reweight(H, s1, s2, self._lnw, temperatures, self.coupling, self.q, self.n_spins)


def potts_multicanonical_scan(size, q, temperatures, walkers: int = 1024, n_iterations: int = 20, sweeps_per_iteration: int = 50,
                              n_production: int = 200, coupling: float = 1.0, periodic=True, seed: int = 0) -> dict:
    """``n_iterations`` weight iterations of ``sweeps_per_iteration`` sweeps from ln W = 0, a production run of ``n_production``
    sweeps with the weights fixed, then :func:`muca_reweight` at ``temperatures``.  Returns its keys plus ``ln_g``, ``weights``,
    ``iterations`` (the per-iteration dictionaries of :meth:`PottsMulticanonical.iterate`) and ``tunnel_events`` (per walker,
    of the production run, between the ends of the range visited by the last iteration)."""
    temperatures = [float(t) for t in temperatures]
    if any(not (math.isfinite(t) and t > 0) for t in temperatures):
        raise ConfigurationError("Temperature must be positive")
    if int(n_iterations) < 0 or int(sweeps_per_iteration) < 1 or int(n_production) < 1:
        raise ValueError("n_iterations must be >= 0, sweeps_per_iteration and n_production >= 1")
    check_muca_model(size, q, walkers, coupling, periodic)
    model = PottsMulticanonical(size, q, walkers, coupling=coupling, periodic=periodic, seed=seed)
    try:
        its = [model.iterate(int(sweeps_per_iteration)) for _ in range(int(n_iterations))]
        if its and its[-1]["range"][0] < its[-1]["range"][1]:
            model.set_tunnel_bounds(*its[-1]["range"])
        model.clear_record().run(int(n_production))
        res = model.reweight(temperatures)
        res["ln_g"] = model.density_of_states()
        res["weights"] = model.weights
        res["iterations"] = its
        res["tunnel_events"] = model.tunnels()
    finally:
        model.close()
    return res

"""Parallel tempering (replica exchange) of Potts lattices with stored couplings and site fields (K13, ``csrc/potts_pt.hip``): the
ladders of :class:`tsu.models.LatticeTempering` for the models of :class:`PottsModel2D` / :class:`PottsModel3D` with ``couplings=`` /
``site_field=``: Potts glasses, random-bond and diluted Potts models, the Potts prior with unary costs.

``ladders`` (1 or 2) ladders of ``R = len(temperatures)`` walkers (2 .. 256) share one disorder.  Walker ``g = k R + w`` of ladder k
has the Philox key ``seed + g``, starts at slot w from ``default_rng(seed + g).integers(0, q, shape)`` (or from one colour) and keeps
its key wherever it goes; the temperature belongs to the slot.  A round = ``swap_interval`` K12 heat-bath sweeps of every walker at
its slot's temperature, every walker's n_eq, N_c and float64 E, one swap pass per ladder by the rule of :class:`LatticeTempering`, and
with two ladders the exact contingency table of the two walkers at every slot -- all on the device, without a host synchronisation.
"""
from typing import Optional

import numpy as np

from .. import _hip
from ..core import ConfigurationError
from .potts import check_potts_temperature, potts_disorder_arrays, potts_order_parameter


def potts_overlap(tables, q: int):
    """The Potts overlap (q sum_a C[a][a] / N - 1) / (q - 1) of contingency tables ``(..., q, q)``: 1 for equal colourings, 0 on
    average for independent ones."""
    tables = np.asarray(tables)
    n = tables.sum(axis=(-2, -1))
    return (q * np.trace(tables, axis1=-2, axis2=-1) / n - 1.0) / (q - 1.0)


def _check_ladder(q, temperatures, ladders, initial):
    """The refusals of a ladder, made on the host before the device is touched: the temperatures as a float64 array."""
    T = np.asarray(temperatures, dtype=np.float64).ravel()
    if not 2 <= T.size <= _hip.POTTS_PT_MAX_TEMPS:
        raise ConfigurationError(f"parallel tempering needs 2 to {_hip.POTTS_PT_MAX_TEMPS} temperatures, got {T.size}")
    for t in T:
        check_potts_temperature(q, t)
    if isinstance(ladders, bool) or ladders not in (1, 2):
        raise ConfigurationError("ladders must be 1 or 2")
    if not (initial == "random" or (not isinstance(initial, (str, bool)) and int(initial) == initial and 0 <= int(initial) < int(q))):
        raise ConfigurationError(f"initial must be 'random' or a colour in 0 .. {int(q) - 1}")
    return T


class _PottsTempering:
    """What :class:`PottsTempering` and :class:`PottsTempering3D` share: everything but the parsing of the shape."""

    def _open(self, q, temperatures, couplings, site_field, coupling, field, seed, initial, ladders):
        self.temperatures = _check_ladder(q, temperatures, ladders, initial)
        self.q, self.ladders = int(q), int(ladders)
        self.n_spins = int(np.prod(self.shape))
        if self.n_spins >= 2 ** 31:
            raise ConfigurationError("the lattice must hold fewer than 2^31 sites")
        per = (self.periodic,) * 2 if len(self.shape) == 2 else tuple(self.periodic)
        if any(p and n % 2 for p, n in zip(per, self.shape)):
            raise ConfigurationError("a periodic axis needs an even length")
        self._J, self._h = potts_disorder_arrays(self.shape, self.q, per, couplings, site_field, coupling, field)
        self.seed = int(seed) if seed is not None else int(np.random.default_rng().integers(0, 2 ** 62))
        R, nw = self.temperatures.size, self.temperatures.size * self.ladders
        if not 0 <= self.seed <= 2 ** 64 - nw:
            raise ConfigurationError(f"seed + {nw} walkers must fit 64 bits")
        self._pt = pt = _hip.PottsTemperingLattice(self.shape, self.q, self.periodic, R, self.ladders)
        try:
            pt.set_disorder(self._J[0], self._J[1], self._J[2] if len(self._J) == 3 else None, self._h)
            pt.set_temperatures(self.temperatures)
            if initial == "random":
                pt.init(self.seed, -1)
                for g in range(nw):
                    pt.set_spins(g // R, g % R, np.random.default_rng(self.seed + g).integers(0, self.q, size=self.shape).astype(np.int8))
            else:
                pt.init(self.seed, int(initial))
        except Exception:
            pt.close()
            raise

    def close(self) -> None:
        self._pt.close()

    def run(self, n_rounds: int, swap_interval: int = 10, swap: bool = True, record: bool = True):
        """n_rounds rounds of swap_interval sweeps each, enqueued without a host synchronisation; with ``record`` returns
        ``history()``, else None."""
        if int(n_rounds) < 0 or int(swap_interval) < 1:
            raise ValueError("n_rounds must be >= 0 and swap_interval >= 1")
        self._pt.run(int(n_rounds), int(swap_interval), swap, record)
        return self.history() if record else None

    def history(self) -> dict:
        """The rounds recorded by the last ``run``, per (ladder, slot): ``E`` (float64), ``n_eq`` (int64 bonds whose ends agree) and
        ``walker`` as (n_rounds, ladders, R), ``N`` (int64 colour counts) as (n_rounds, ladders, R, q).  With two ladders also
        ``tables``: int64 (n_rounds, R, q, q), ``tables[t, i, a, b]`` the sites that show colour a in ladder 0's walker and b in ladder
        1's walker at slot i, and ``overlap`` = :func:`potts_overlap` of them."""
        h = self._pt.history()
        if h["tables"] is None:
            del h["tables"]
        else:
            h["overlap"] = potts_overlap(h["tables"], self.q) if len(h["tables"]) else np.zeros(h["tables"].shape[:2])
        return h

    @property
    def swap_acceptance(self) -> np.ndarray:
        """Accepted / attempted swaps per adjacent pair of slots, ladders pooled (NaN before the first attempt)."""
        st = self._pt.stats()
        with np.errstate(divide="ignore", invalid="ignore"):
            return st["accepts"].sum(axis=0) / st["attempts"].sum(axis=0)

    @property
    def round_trips(self) -> int:
        """Round trips (slot 0 -> last slot -> slot 0) completed by all walkers of all ladders."""
        return int(self._pt.stats()["round_trips"].sum())

    @property
    def walker_at_slot(self) -> np.ndarray:
        """(ladders, R): which walker sits at each slot."""
        return self._pt.stats()["walker_at_slot"]

    @property
    def sweep_count(self) -> int:
        return int(self._pt.stats()["sweep_count"])

    def stats(self) -> dict:
        """attempts, accepts (ladders, R - 1); round_trips (ladders, R) by walker; walker_at_slot; sweep_count; round_count."""
        return self._pt.stats()

    def energies(self) -> np.ndarray:
        """float64 E of every walker now, (ladders, R) indexed by walker: the bits of that lattice's ``PottsModel*.energy()``."""
        return self._pt.energies()[0]

    def spins(self, ladder: int, slot: int) -> np.ndarray:
        """Colours of the walker now at ``(ladder, slot)``, in the lattice's shape."""
        if not (0 <= slot < self.temperatures.size and 0 <= ladder < self.ladders):
            raise ValueError(f"slot {slot} / ladder {ladder} out of range ({self.ladders} ladder(s) of {self.temperatures.size})")
        return self._pt.get_spins(ladder, slot)

    def route(self) -> str:
        return self._pt.route()

    def launch_count(self) -> int:
        return self._pt.launch_count()


class PottsTempering(_PottsTempering):
    """Parallel tempering of a 2-D Potts lattice with stored couplings (module docstring).  ``size``: an edge or (rows, cols);
    ``couplings=(J_right, J_down)`` and ``site_field`` (shape + (q,)) as for :class:`PottsModel2D`, or the uniform ``coupling`` and
    per-colour ``field``; everything is checked and rounded to float32 before any device call.  Without swaps walker g equals
    ``PottsModel2D(seed=seed + g, temperature=T[g % R])`` on the same disorder bit for bit, energies included."""

    def __init__(self, size, q, temperatures, *, couplings=None, site_field=None, coupling: float = 1.0, field=None,
                 periodic: bool = True, seed: Optional[int] = None, initial="random", ladders: int = 1):
        self.shape = (int(size), int(size)) if np.isscalar(size) else tuple(int(v) for v in size)
        if len(self.shape) != 2 or min(self.shape) < 1:
            raise ConfigurationError("size must be a positive edge or (rows, cols)")
        self.rows, self.cols = self.shape
        self.periodic = bool(periodic)
        self._open(q, temperatures, couplings, site_field, coupling, field, seed, initial, ladders)


class PottsTempering3D(_PottsTempering):
    """:class:`PottsTempering` on the cubic lattice: ``size`` an edge or (D, R, C), ``couplings=(J_right, J_down, J_layer)``,
    ``periodic`` a bool (all three axes) or ``(p_z, p_r, p_c)``.  Without swaps walker g equals
    ``PottsModel3D(seed=seed + g, temperature=T[g % R])``."""

    def __init__(self, size, q, temperatures, *, couplings=None, site_field=None, coupling: float = 1.0, field=None,
                 periodic=True, seed: Optional[int] = None, initial="random", ladders: int = 1):
        self.shape = (int(size),) * 3 if np.isscalar(size) else tuple(int(v) for v in size)
        if len(self.shape) != 3 or min(self.shape) < 1:
            raise ConfigurationError("size must be a positive edge or (depth, rows, cols)")
        self.depth, self.rows, self.cols = self.shape
        try:
            self.periodic = _hip.periodic_axes(periodic)
        except ValueError as e:
            raise ConfigurationError(str(e)) from None
        self._open(q, temperatures, couplings, site_field, coupling, field, seed, initial, ladders)


def _scan(cls, size, q, temperatures, coupling, n_equilibrate, n_measure, measure_every, periodic, seed, couplings, site_field,
          replicas, swap) -> dict:
    if replicas not in (1, 2):
        raise ValueError("replicas must be 1 or 2")
    if int(n_measure) < 1 or int(measure_every) < 1 or int(n_equilibrate) < 0:
        raise ValueError("n_measure and measure_every must be >= 1, n_equilibrate >= 0")
    if int(n_equilibrate) % int(measure_every):
        raise ValueError("n_equilibrate must be a multiple of measure_every")
    pt = cls(size, q, temperatures, couplings=couplings, site_field=site_field, coupling=coupling, periodic=periodic, seed=seed,
             ladders=replicas)
    try:
        pt.run(int(n_equilibrate) // int(measure_every), int(measure_every), swap=swap, record=False)
        hist = pt.run(int(n_measure), int(measure_every), swap=swap, record=True)
        N, T = pt.n_spins, pt.temperatures
        e = hist["E"][:, 0].T / N  # (R, n_measure), the walker at each slot
        m = potts_order_parameter(hist["N"][:, 0], int(q)).T
        m2 = np.mean(m ** 2, axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            out = {"energy": e.mean(axis=1), "order_parameter": m.mean(axis=1), "specific_heat": N * e.var(axis=1) / T ** 2,
                   "susceptibility": N * m.var(axis=1) / T,
                   "binder": np.where(m2 > 0, 1.0 - np.mean(m ** 4, axis=1) / (3.0 * m2 ** 2), np.nan), "temperatures": T.copy()}
            if replicas == 2:
                ov = hist["overlap"].T
                o2 = np.mean(ov ** 2, axis=1)
                out["overlap"] = ov.mean(axis=1)
                out["overlap_sq"] = o2
                out["overlap_binder"] = np.where(o2 > 0, 1.0 - np.mean(ov ** 4, axis=1) / (3.0 * o2 ** 2), np.nan)
        out["swap_acceptance"] = pt.swap_acceptance
        out["round_trips"] = pt.round_trips
    finally:
        pt.close()
    return out


def potts_tempering_scan(size, q, temperatures, coupling: float = 1.0, n_equilibrate: int = 1000, n_measure: int = 50,
                         measure_every: int = 10, periodic: bool = True, seed: int = 0, *, couplings=None, site_field=None,
                         replicas: int = 1, swap: bool = True) -> dict:
    """:func:`potts_temperature_scan` of a lattice with stored couplings, with replica exchange between the temperatures
    (:class:`PottsTempering`).  One round = ``measure_every`` heat-bath sweeps of every walker + one swap pass; ``n_equilibrate`` (a
    multiple of ``measure_every``) sweeps of rounds, then ``n_measure`` recorded rounds.  Returns potts_temperature_scan's keys,
    computed by the same expressions from the walker at each temperature, plus ``swap_acceptance`` (per adjacent pair, ladders
    pooled) and ``round_trips`` (all walkers); with ``replicas=2`` also ``overlap``, ``overlap_sq`` and ``overlap_binder`` =
    1 - <Q^4> / (3 <Q^2>^2) of the Potts overlap Q of the two replicas at each temperature.

    ``potts_temperature_scan`` seeds every temperature with the same ``seed``; the ladder's walker g is
    ``PottsModel2D(seed=seed + g, temperature=T[g])``.  So ``swap=False`` equals those models, not the scan."""
    return _scan(PottsTempering, size, q, temperatures, coupling, n_equilibrate, n_measure, measure_every, periodic, seed, couplings,
                 site_field, replicas, swap)


def potts_tempering_scan_3d(size, q, temperatures, coupling: float = 1.0, n_equilibrate: int = 1000, n_measure: int = 50,
                            measure_every: int = 10, periodic=True, seed: int = 0, *, couplings=None, site_field=None,
                            replicas: int = 1, swap: bool = True) -> dict:
    """:func:`potts_tempering_scan` on the cubic lattice (:class:`PottsTempering3D`): the same keys.  The ladder's walker g is
    ``PottsModel3D(seed=seed + g, temperature=T[g])``, not a model of ``potts_temperature_scan_3d`` (which seeds every temperature
    with the same ``seed``)."""
    return _scan(PottsTempering3D, size, q, temperatures, coupling, n_equilibrate, n_measure, measure_every, periodic, seed,
                 couplings, site_field, replicas, swap)

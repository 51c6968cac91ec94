"""Population annealing of Potts lattices with stored couplings and site fields (K14, ``csrc/potts_pop.hip``): the populations of
:class:`tsu.models.PopulationAnnealing` for the models of :class:`PottsModel2D` / :class:`PottsModel3D` with ``couplings=`` /
``site_field=``: Potts glasses, random-bond and diluted Potts models, antiferromagnetic Potts models, the Potts prior with unary
costs.  It is the one method here that yields ln Z, the free energy and the entropy of such a model, and it keeps the lowest-energy
colouring the population holds.

``population`` walkers (2 .. 65535) share one disorder and one temperature.  Walker i has the Philox key ``seed + i`` and the shared
sweep counter; the key belongs to the index, so copies diverge.  A step reweights the population from beta[k-1] to beta[k] by
systematic resampling at fixed size with 30-bit integer weights, copies the colours of the walkers that multiply over those that die,
sweeps every walker ``sweeps_per_step`` times with K12's heat bath at 1 / beta[k] and measures every walker's float64 E, n_eq and
colour counts -- all on the device, without a host synchronisation.  Small lattices are swept several walkers to a workgroup, the
disorder staged in LDS (``route()``, ``plan()``).
"""
from typing import Optional

import numpy as np

from .. import _hip
from ..core import ConfigurationError
from .ising import POPULATION_WEIGHT_ONE, _check_population, _population_schedule, population_family_stats
from .potts import check_potts_temperature, potts_disorder_arrays, potts_order_parameter


def potts_population_free_energy(betas, S, E_min, mean_E, population: int, n_spins: int, q: int) -> dict:
    """:func:`tsu.models.ising.population_free_energy` for q states a site: step j multiplies the partition function by Q_j with
    ``ln Q_j = -db_j E_min_j + ln(S_j / (R 2^30))``; ``ln_Z[k] = N ln q + sum_{j <= k} ln Q_j`` when ``betas[0] == 0`` (the uniform
    measure), else the difference ``ln Z(betas[k]) - ln Z(betas[0])``.  ``F = -ln_Z / beta`` and ``entropy = beta <E> + ln_Z`` (NaN
    where beta[0] > 0 leaves only differences; F is NaN at beta = 0)."""
    betas = np.asarray(betas, dtype=float)
    db = np.diff(betas)
    lnQ = -db * np.asarray(E_min, dtype=float) + np.log(np.asarray(S, dtype=float) / (float(population) * POPULATION_WEIGHT_ONE))
    absolute = betas[0] == 0.0
    ln_Z = np.concatenate([[0.0], np.cumsum(lnQ)]) + (n_spins * np.log(float(q)) if absolute else 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        F = np.where(betas > 0, -ln_Z / betas, np.nan) if absolute else np.full(betas.size, np.nan)
    entropy = betas * np.asarray(mean_E, dtype=float) + ln_Z if absolute else np.full(betas.size, np.nan)
    return {"betas": betas, "ln_Q": lnQ, "ln_Z": ln_Z, "F": F, "entropy": entropy}


_ROWS_PLUS_ONE = ("E", "n_eq", "N")  # keys whose row 0 is the population a run started from


class _PottsPopulationAnnealing:
    """What :class:`PottsPopulationAnnealing` and :class:`PottsPopulationAnnealing3D` share: everything but the parsing of the shape."""

    def _open(self, q, population, betas, temperatures, couplings, site_field, coupling, field, seed, initial, sweeps_per_step,
              initial_sweeps):
        check_potts_temperature(q, 1.0)
        self.q = int(q)
        self.population = _check_population(population)
        self.betas = _population_schedule(betas, temperatures)
        if int(sweeps_per_step) < 0 or int(initial_sweeps) < 0:
            raise ValueError("sweeps_per_step and initial_sweeps must be >= 0")
        self.sweeps_per_step, self.initial_sweeps = int(sweeps_per_step), int(initial_sweeps)
        if not (initial == "random" or (not isinstance(initial, (str, bool)) and int(initial) == initial and 0 <= int(initial) < self.q)):
            raise ConfigurationError(f"initial must be 'random' or a colour in 0 .. {self.q - 1}")
        self.n_spins = int(np.prod(self.shape))
        if self.n_spins >= 2 ** 31:
            raise ConfigurationError("the lattice must hold fewer than 2^31 sites")
        per = (self.periodic,) * 2 if len(self.shape) == 2 else tuple(self.periodic)
        if any(p and n % 2 for p, n in zip(per, self.shape)):
            raise ConfigurationError("a periodic axis needs an even length")
        self._J, self._h = potts_disorder_arrays(self.shape, self.q, per, couplings, site_field, coupling, field)
        self.seed = int(seed) if seed is not None else int(np.random.default_rng().integers(0, 2 ** 62))
        if not 0 <= self.seed <= 2 ** 64 - self.population:
            raise ConfigurationError(f"seed + {self.population} walkers must fit 64 bits")
        self._pa = pa = _hip.PottsPopulation(self.shape, self.q, self.periodic, self.population)
        try:
            pa.set_disorder(self._J[0], self._J[1], self._J[2] if len(self._J) == 3 else None, self._h)
            pa.set_schedule(self.betas)
            pa.init(self.seed, _hip.POTTS_POP_DRAW if initial == "random" else int(initial), self.initial_sweeps)
        except Exception:
            pa.close()
            raise
        self.step_count = 0
        self.sweep_count = self.initial_sweeps if self.betas[0] > 0 else 0
        self._record = None    # the rows since init while every run recorded, else None
        self._complete = True  # no run since init went unrecorded

    def close(self) -> None:
        self._pa.close()

    @property
    def n_steps(self) -> int:
        """Steps of the schedule."""
        return self.betas.size - 1

    def run(self, n_steps: Optional[int] = None, resample: bool = True, record: bool = True):
        """``n_steps`` further steps of the schedule (default: all that are left); with ``record`` returns ``history()``."""
        left = self.n_steps - self.step_count
        n = left if n_steps is None else int(n_steps)
        if not 0 <= n <= left:
            raise ValueError(f"n_steps = {n} runs past the schedule ({left} of {self.n_steps} steps left)")
        self._pa.run(n, self.sweeps_per_step, resample, record)
        self.step_count += n
        self.sweep_count += n * self.sweeps_per_step
        if not record:
            self._complete, self._record = False, None
            return None
        h = self._pa.history()
        h["resampled"] = np.full(n, bool(resample))
        if self._complete:
            if self._record is None:
                self._record = h
            else:  # row 0 of a later run repeats the last row of the one before
                r = self._record
                self._record = {k: np.concatenate([r[k], h[k][1:] if k in _ROWS_PLUS_ONE else h[k]]) for k in h}
        else:
            self._last = h
        return self.history()

    def history(self) -> dict:
        """Every step since the start, if every run recorded (else the last run's steps): ``E`` (float64), ``n_eq`` (int64 bonds
        whose ends agree) as (n + 1, R) and ``N`` (int64 colour counts) as (n + 1, R, q) by walker index, row 0 the start; ``W``
        (uint32 weights), ``parent`` (int32) (n, R); ``S``, ``U`` (uint64), ``E_min`` (n,); ``resampled`` (n,) bool.  Steps taken with
        ``resample=False`` have ``parent`` = identity and zeros in ``W``, ``S``, ``U``, ``E_min``."""
        if self._complete and self._record is not None:
            return dict(self._record)
        if self._complete:
            raise ValueError("history: nothing has been recorded yet")
        return dict(self._last)

    def _full_record(self, what):
        if not (self._complete and self._record is not None):
            raise ValueError(f"{what} needs the record of every step since the start: run with record=True throughout")
        return self._record

    def free_energy(self) -> dict:
        """``ln_Z``, ``F`` and ``entropy`` at every recorded beta (:func:`potts_population_free_energy`: ``ln_Z[0] = N ln q`` when
        beta[0] = 0); needs resampled steps."""
        r = self._full_record("free_energy")
        if not np.all(r["resampled"]):
            raise ValueError("free_energy needs resampled steps (run(resample=True))")
        k = r["S"].size
        return potts_population_free_energy(self.betas[:k + 1], r["S"], r["E_min"], r["E"].mean(axis=1), self.population, self.n_spins,
                                            self.q)

    def observables(self) -> dict:
        """Population means per recorded beta: ``energy`` (<E>), ``energy_sq``, ``equal_bonds`` (<n_eq>), ``order_parameter``
        (<m>, m = (q max_c N_c / N - 1) / (q - 1)) and ``order_parameter_sq``, with ``betas``."""
        r = self._full_record("observables")
        m = potts_order_parameter(r["N"], self.q)
        return {"betas": self.betas[:r["E"].shape[0]], "energy": r["E"].mean(axis=1), "energy_sq": (r["E"] ** 2).mean(axis=1),
                "equal_bonds": r["n_eq"].mean(axis=1), "order_parameter": m.mean(axis=1), "order_parameter_sq": (m ** 2).mean(axis=1)}

    def family_stats(self) -> dict:
        """``rho_t``, ``rho_s`` and ``families`` per recorded beta (:func:`tsu.models.ising.population_family_stats`)."""
        return population_family_stats(self._full_record("family_stats")["parent"])

    def spins(self, i: int) -> np.ndarray:
        """Colours of walker ``i``, in the lattice's shape."""
        if not 0 <= i < self.population:
            raise ValueError(f"walker {i} out of range (population {self.population})")
        return self._pa.get_spins(i)

    def energies(self) -> np.ndarray:
        """Every walker's energy now: the bits of that lattice's ``PottsModel*.energy()``."""
        return self._pa.energies()[0]

    def best(self):
        """``(E, colours)`` of the lowest-energy walker now, the lowest index on ties."""
        E = self.energies()
        i = int(np.argmin(E))
        return float(E[i]), self.spins(i)

    def route(self) -> str:
        return self._pa.route()

    def plan(self) -> dict:
        """What the packing rule gives this population: ``route``, ``G`` walkers a workgroup, ``threads`` and ``lds_bytes``."""
        return self._pa.plan()

    def launch_count(self) -> int:
        return self._pa.launch_count()


class PottsPopulationAnnealing(_PottsPopulationAnnealing):
    """Population annealing of a 2-D Potts lattice with stored couplings (module docstring).  ``size``: an edge or (rows, cols);
    ``couplings=(J_right, J_down)`` and ``site_field`` (shape + (q,)) as for :class:`PottsModel2D`, or the uniform ``coupling`` and
    per-colour ``field``; the schedule is exactly one of ``betas`` (ascending, first >= 0) and ``temperatures`` (descending, ``inf``
    allowed first).  Everything is checked and rounded to float32 before any device call.

    ``initial="random"`` draws every walker on the device from its own Philox key (uniform colours to within q 2^-32); it is NOT the
    host draw ``default_rng(seed).integers`` of :class:`PottsModel2D`.  A first beta of 0 makes that draw the equilibrium start; a
    larger one takes ``initial_sweeps`` sweeps there.  ``run(resample=False)`` anneals the walkers independently: walker i then
    equals ``PottsModel2D(seed=seed + i, temperature=1 / beta[k])`` started from the walker's colours, bit for bit, energies
    included."""

    def __init__(self, size, q, population, *, betas=None, temperatures=None, couplings=None, site_field=None, coupling: float = 1.0,
                 field=None, periodic: bool = True, seed: Optional[int] = None, initial="random", sweeps_per_step: int = 10,
                 initial_sweeps: int = 0):
        self.shape = (int(size), int(size)) if np.isscalar(size) else tuple(int(v) for v in size)
        if len(self.shape) != 2 or min(self.shape) < 1:
            raise ConfigurationError("size must be a positive edge or (rows, cols)")
        self.rows, self.cols = self.shape
        self.periodic = bool(periodic)
        self._open(q, population, betas, temperatures, couplings, site_field, coupling, field, seed, initial, sweeps_per_step, initial_sweeps)


class PottsPopulationAnnealing3D(_PottsPopulationAnnealing):
    """:class:`PottsPopulationAnnealing` on the cubic lattice: ``size`` an edge or (D, R, C), ``couplings=(J_right, J_down,
    J_layer)``, ``periodic`` a bool (all three axes) or ``(p_z, p_r, p_c)``.  ``initial="random"`` is the device draw, not
    :class:`PottsModel3D`'s host draw."""

    def __init__(self, size, q, population, *, betas=None, temperatures=None, couplings=None, site_field=None, coupling: float = 1.0,
                 field=None, periodic=True, seed: Optional[int] = None, initial="random", sweeps_per_step: int = 10,
                 initial_sweeps: int = 0):
        self.shape = (int(size),) * 3 if np.isscalar(size) else tuple(int(v) for v in size)
        if len(self.shape) != 3 or min(self.shape) < 1:
            raise ConfigurationError("size must be a positive edge or (depth, rows, cols)")
        self.depth, self.rows, self.cols = self.shape
        try:
            self.periodic = _hip.periodic_axes(periodic)
        except ValueError as e:
            raise ConfigurationError(str(e)) from None
        self._open(q, population, betas, temperatures, couplings, site_field, coupling, field, seed, initial, sweeps_per_step, initial_sweeps)


def _scan(pa) -> dict:
    """The body of the scans on a fresh population ``pa``, closed at the end: the whole schedule, then per temperature the keys a
    single replica of :func:`potts_tempering_scan` has, as population means, plus the free energy and the family statistics."""
    try:
        h = pa.run()
        N, q = pa.n_spins, pa.q
        with np.errstate(divide="ignore"):
            T = 1.0 / pa.betas
        e = h["E"] / N
        m = potts_order_parameter(h["N"], q)
        m2 = np.mean(m ** 2, axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            out = {"energy": e.mean(axis=1), "order_parameter": m.mean(axis=1), "specific_heat": N * e.var(axis=1) / T ** 2,
                   "susceptibility": N * m.var(axis=1) / T,
                   "binder": np.where(m2 > 0, 1.0 - np.mean(m ** 4, axis=1) / (3.0 * m2 ** 2), np.nan), "temperatures": T}
        out["betas"] = pa.betas.copy()
        fe = pa.free_energy()
        out["ln_Z"], out["F"], out["entropy"] = fe["ln_Z"], fe["F"], fe["entropy"]
        fam = pa.family_stats()
        out["rho_t"], out["rho_s"] = fam["rho_t"], fam["rho_s"]
    finally:
        pa.close()
    return out


def potts_population_annealing_scan(size, q, population, *, betas=None, temperatures=None, coupling: float = 1.0, couplings=None,
                                    site_field=None, periodic: bool = True, seed: int = 0, sweeps_per_step: int = 10,
                                    initial_sweeps: int = 0) -> dict:
    """``energy``, ``order_parameter``, ``specific_heat``, ``susceptibility``, ``binder`` and ``temperatures`` per temperature of the
    schedule (:func:`potts_tempering_scan`'s expressions, as population means of one :class:`PottsPopulationAnnealing` run), plus
    ``betas``, ``ln_Z``, ``F``, ``entropy`` (differences from the first beta, and NaN, unless it is 0), ``rho_t`` and ``rho_s``."""
    return _scan(PottsPopulationAnnealing(size, q, population, betas=betas, temperatures=temperatures, couplings=couplings,
                                          site_field=site_field, coupling=coupling, periodic=periodic, seed=seed,
                                          sweeps_per_step=sweeps_per_step, initial_sweeps=initial_sweeps))


def potts_population_annealing_scan_3d(size, q, population, *, betas=None, temperatures=None, coupling: float = 1.0, couplings=None,
                                       site_field=None, periodic=True, seed: int = 0, sweeps_per_step: int = 10,
                                       initial_sweeps: int = 0) -> dict:
    """:func:`potts_population_annealing_scan` on the cubic lattice (:class:`PottsPopulationAnnealing3D`): the same keys."""
    return _scan(PottsPopulationAnnealing3D(size, q, population, betas=betas, temperatures=temperatures, couplings=couplings,
                                            site_field=site_field, coupling=coupling, periodic=periodic, seed=seed,
                                            sweeps_per_step=sweeps_per_step, initial_sweeps=initial_sweeps))

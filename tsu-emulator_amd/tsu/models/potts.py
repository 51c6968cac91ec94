"""q-state Potts lattices in 2-D and 3-D (K10): the categorical counterparts of :class:`IsingModel2D` and :class:`IsingModel3D`.

The reference names categorical cells (``ThermalSamplingUnit.sample_categorical``, tsu/core.py) and has no lattice of them; this
module is the package's own.  Site (r, c) holds a colour 0 .. q - 1; E = -J n_eq - sum_c h_c N_c with n_eq the bonds whose two ends
agree and N_c the sites of colour c.  Heat-bath sweeps take J of either sign and a per-colour field; Swendsen-Wang steps need J > 0
and a zero field.  Everything runs in ``csrc/potts2d.hip`` and ``csrc/potts3d.hip``; the initial colours come from NumPy on the host.

With ``couplings=(J_right, J_down[, J_layer])`` and / or ``site_field=`` (shape + (q,)) a model lives on K12's handle instead
(``csrc/potts_disorder.hip``): E = -sum_bonds J_b [s_i = s_j] - sum_i h[i][s_i], the random-bond and diluted Potts models and the Potts
prior with unary costs.  Heat-bath sweeps take any couplings and fields; Swendsen-Wang steps need every coupling >= 0 and a zero field.
"""
import math
from typing import Optional

import numpy as np

from .. import _hip
from ..core import ConfigurationError

ALGORITHMS = {"heat_bath": _hip.POTTS_HEAT_BATH, "swendsen_wang": _hip.POTTS_SWENDSEN_WANG}


def check_potts_model(q, coupling, field, temperature, neighbours: int = 4):
    """The refusals of the model, made on the host before the device is touched; returns the field as a float64 array of q values.
    ``neighbours``: 4 on the square lattice, 6 on the cubic one (whatever its depth)."""
    if isinstance(q, bool) or int(q) != q or not 2 <= int(q) <= _hip.POTTS_MAX_Q:
        raise ConfigurationError(f"q must be an integer in 2 .. {_hip.POTTS_MAX_Q} (got {q!r})")
    q = int(q)
    h = np.zeros(q) if field is None else np.array(field, dtype=np.float64)
    if h.shape != (q,):
        raise ConfigurationError(f"field must hold q = {q} values, one per colour")
    J, T = float(coupling), float(temperature)
    if not (math.isfinite(J) and math.isfinite(T) and np.all(np.isfinite(h))):
        raise ConfigurationError("coupling, field and temperature must be finite")
    if not T > 0:
        raise ConfigurationError("Temperature must be positive")
    if (float(neighbours) * abs(J) + float(h.max() - h.min())) / T > 600.0:
        raise ConfigurationError(f"({neighbours} |J| + max h - min h) / T exceeds 600: the heat-bath weights would leave the float64 range")
    return h


def check_potts_temperature(q, temperature) -> None:
    """The refusals of a model with stored couplings: q and T only (its weights are normalised per site, so no bound on J / T)."""
    if isinstance(q, bool) or int(q) != q or not 2 <= int(q) <= _hip.POTTS_MAX_Q:
        raise ConfigurationError(f"q must be an integer in 2 .. {_hip.POTTS_MAX_Q} (got {q!r})")
    T = float(temperature)
    if not math.isfinite(T):
        raise ConfigurationError("coupling, field and temperature must be finite")
    if not T > 0:
        raise ConfigurationError("Temperature must be positive")


def _fp32(name, a, shape):
    """``a`` as a float32 array of ``shape``, rounded once; non-finite values and fp32 overflow are refused."""
    a = np.asarray(a, dtype=np.float64)
    if a.shape != tuple(shape):
        raise ConfigurationError(f"{name} must have shape {tuple(shape)} (got {a.shape})")
    if not np.all(np.isfinite(a)):
        raise ConfigurationError(f"{name} must be finite")
    with np.errstate(over="ignore"):
        a32 = a.astype(np.float32)
    if not np.all(np.isfinite(a32)):
        raise ConfigurationError(f"{name} overflows float32")
    return np.ascontiguousarray(a32)


def potts_disorder_arrays(shape, q, periodic, couplings=None, site_field=None, coupling: float = 1.0, field=None):
    """The disorder of a K12 model as the device takes it, checked on the host: ``(J arrays, h)`` with one fp32 array of the
    lattice's shape per axis in the order (J_right, J_down[, J_layer]) and h colour-major, ``(q,) + shape`` fp32, or None for no
    field.  ``periodic``: one flag per axis of ``shape``, in its order.  Without ``couplings`` every existing bond is ``coupling``;
    without ``site_field`` the per-colour ``field`` (if any is non-zero) is spread over the sites.  On an open axis the last slice
    of that axis's array must be 0."""
    shape = tuple(int(n) for n in shape)
    nd = len(shape)
    names = ("J_right", "J_down", "J_layer")[:nd]
    if couplings is None:
        J = float(coupling)
        if not math.isfinite(J):
            raise ConfigurationError("coupling, field and temperature must be finite")
        arrs = []
        for k in range(nd):
            a = np.full(shape, J, np.float64)
            if not periodic[nd - 1 - k]:
                a[(slice(None),) * (nd - 1 - k) + (-1,)] = 0.0
            arrs.append(a)
        couplings = arrs
    else:
        if float(coupling) != 1.0:
            raise ConfigurationError("give either coupling or couplings, not both")
        couplings = tuple(couplings)
        if len(couplings) != nd:
            raise ConfigurationError(f"couplings must hold {nd} arrays: " + ", ".join(names))
    out = []
    for k, (name, a) in enumerate(zip(names, couplings)):
        a32 = _fp32(name, a, shape)
        axis = nd - 1 - k  # J_right runs along the last axis
        if not periodic[axis] and np.any(a32[(slice(None),) * axis + (-1,)] != 0):
            raise ConfigurationError(f"open axis: the last slice of {name} along axis {axis} must be 0")
        out.append(a32)
    if site_field is not None:
        if field is not None and np.any(np.asarray(field, dtype=np.float64) != 0):
            raise ConfigurationError("give either field or site_field, not both")
        h = np.ascontiguousarray(np.moveaxis(_fp32("site_field", site_field, shape + (int(q),)), -1, 0))
    elif field is not None and np.any(np.asarray(field, dtype=np.float64) != 0):
        f32 = _fp32("field", field, (int(q),))
        h = np.ascontiguousarray(np.broadcast_to(f32.reshape((int(q),) + (1,) * nd), (int(q),) + shape))
    else:
        h = None
    return tuple(out), h


def _algorithm(name: str) -> int:
    if name not in ALGORITHMS:
        raise ValueError("algorithm must be 'heat_bath' or 'swendsen_wang'")
    return ALGORITHMS[name]


class _PottsLattice:
    """What the 2-D and the 3-D model share: everything but the constructor.  A subclass sets ``shape``, ``_neighbours`` and ``_lat``."""

    _neighbours = 4
    _disordered = False  # True: the model lives on K12's handle (couplings= / site_field= were given)

    def _periodic_axes(self):
        return (self.periodic,) * 2 if len(self.shape) == 2 else tuple(self.periodic)

    def _open_disorder(self, couplings, site_field) -> None:
        """Checks the arrays on the host, then creates K12's handle and hands them over."""
        self._J, self._h = potts_disorder_arrays(self.shape, self.q, self._periodic_axes(), couplings, site_field, self.coupling, self.field)
        self._disordered = True
        self._lat = _hip.PottsDisorderLattice(self.shape, self.q, self.periodic)
        self._lat.set_disorder(self._J[0], self._J[1], self._J[2] if len(self._J) == 3 else None, self._h)

    def set_disorder(self, couplings=None, site_field=None):
        """New couplings and / or a new site field for a model built with ``couplings=`` or ``site_field=``; what is not given
        stays.  Checked on the host before the device is touched."""
        if not self._disordered:
            raise ConfigurationError("set_disorder needs a model built with couplings= or site_field=")
        J, h = potts_disorder_arrays(self.shape, self.q, self._periodic_axes(), self._J if couplings is None else couplings,
                                     site_field)
        if site_field is None:
            h = self._h
        self._lat.set_disorder(J[0], J[1], J[2] if len(J) == 3 else None, h)
        self._J, self._h = J, h
        return self

    def close(self) -> None:
        self._lat.close()

    @property
    def spins(self) -> np.ndarray:
        return self._lat.get_spins()

    @spins.setter
    def spins(self, colours) -> None:
        s = np.asarray(colours)
        if s.shape != self.shape:
            raise ValueError(f"spins must have shape {self.shape}")
        if not np.issubdtype(s.dtype, np.integer) or s.min() < 0 or s.max() >= self.q:
            raise ValueError(f"spins must be integer colours in 0 .. {self.q - 1}")
        self._lat.set_spins(s.astype(np.int8))

    def fill(self, colour: int):
        if not 0 <= int(colour) < self.q:
            raise ValueError(f"colour must be in 0 .. {self.q - 1}")
        self._lat.fill(int(colour))
        return self

    def _set_temperature(self, temperature) -> None:
        if temperature is not None:
            if self._disordered:
                check_potts_temperature(self.q, temperature)
            else:
                check_potts_model(self.q, self.coupling, self.field, temperature, self._neighbours)
            self.temperature = float(temperature)

    def gibbs_update(self, n_sweeps: int = 1):
        self._lat.sweep(self.temperature, int(n_sweeps), self.seed, self.sweep_count & 0xFFFFFFFF)
        self.sweep_count += int(n_sweeps)
        return self

    def cluster_update(self, n_steps: int = 1):
        """n Swendsen-Wang steps; :class:`tsu._hip.UnsupportedError` for J <= 0 or a field, the state untouched."""
        self._lat.cluster_sweep(self.temperature, int(n_steps), self.seed, self.cluster_count)
        self.cluster_count += int(n_steps)
        return self

    def equilibrate(self, temperature: Optional[float] = None, n_sweeps: int = 1000, algorithm: str = "heat_bath"):
        alg = _algorithm(algorithm)
        self._set_temperature(temperature)
        return self.cluster_update(n_sweeps) if alg == _hip.POTTS_SWENDSEN_WANG else self.gibbs_update(n_sweeps)

    def run(self, n_measure: int, measure_every: int = 1, algorithm: str = "heat_bath") -> np.ndarray:
        """``n_measure`` times ``measure_every`` updates and one measurement, without a host round trip in between: the
        ``(n_measure, 1 + q)`` int64 rows (n_eq, N_0 .. N_{q-1}).  The counters run on as for the single calls.  A model with stored
        couplings returns ``(rows, E)``: the float64 energy of every measurement as well."""
        alg = _algorithm(algorithm)
        sw = alg == _hip.POTTS_SWENDSEN_WANG
        self._lat.run(self.temperature, int(n_measure), int(measure_every), alg, self.seed,
                      self.cluster_count if sw else self.sweep_count & 0xFFFFFFFF)
        if sw:
            self.cluster_count += int(n_measure) * int(measure_every)
        else:
            self.sweep_count += int(n_measure) * int(measure_every)
        if self._disordered:
            rows, E = self._lat.record()
            return rows[:, :1 + self.q], E
        return self._lat.record()[:, :1 + self.q]

    def colour_counts(self) -> np.ndarray:
        return self._lat.measure()[1]

    def equal_bonds(self) -> int:
        return self._lat.measure()[0]

    def energy(self) -> float:
        if self._disordered:
            return self._lat.measure()[2]
        n_eq, N = self._lat.measure()
        return -self.coupling * n_eq - float(np.dot(self.field, N))

    def order_parameter(self) -> float:
        return float(potts_order_parameter(self.colour_counts(), self.q))

    def route(self, algorithm: str = "heat_bath") -> str:
        return self._lat.route(_algorithm(algorithm))

    def launch_count(self) -> int:
        return self._lat.launch_count()


class PottsModel2D(_PottsLattice):
    """A q-state Potts lattice that lives on the GPU between calls.

    ``gibbs_update(n)`` = n checkerboard heat-bath sweeps (counter ``sweep_count``); ``cluster_update(n)`` = n Swendsen-Wang steps
    (J > 0, zero field; counter ``cluster_count``); ``energy()``, ``colour_counts()`` and ``order_parameter()`` come from exact
    integers reduced on the device.  ``spins`` is an int8 array of colours 0 .. q - 1.
    """

    def __init__(self, size, q, temperature: float = 1.0, coupling: float = 1.0, field=None, periodic: bool = True,
                 seed: Optional[int] = None, *, couplings=None, site_field=None):
        disordered = couplings is not None or site_field is not None
        if disordered:
            check_potts_temperature(q, temperature)
            self.field = None if field is None else np.array(field, dtype=np.float64)
        else:
            self.field = check_potts_model(q, coupling, field, temperature)
        self.q = int(q)
        self.rows, self.cols = (int(size), int(size)) if np.isscalar(size) else tuple(int(v) for v in size)
        if self.rows < 1 or self.cols < 1:
            raise ConfigurationError("size must be positive")
        self.periodic = bool(periodic)
        if self.periodic and (self.rows % 2 or self.cols % 2):
            raise ConfigurationError("a periodic lattice needs even rows and columns")
        self.shape = (self.rows, self.cols)
        self.n_spins = self.rows * self.cols
        self.coupling = float(coupling)
        self.temperature = float(temperature)
        self.seed = int(seed) if seed is not None else int(np.random.default_rng().integers(0, 2 ** 63))
        self.sweep_count = 0
        self.cluster_count = 0
        if disordered:
            self._open_disorder(couplings, site_field)
        else:
            self._lat = _hip.PottsLattice(self.rows, self.cols, self.q, self.periodic)
            self._lat.set_model(self.coupling, self.field)
        self._lat.set_spins(np.random.default_rng(self.seed).integers(0, self.q, size=(self.rows, self.cols)).astype(np.int8))


class PottsModel3D(_PottsLattice):
    """A q-state Potts lattice on the cubic lattice, ``size`` = (D, R, C) or one edge; ``periodic`` a bool (all three axes) or
    ``(p_z, p_r, p_c)``; a periodic axis needs an even length, an open one any length >= 1 (one layer: D = 1 with an open z axis,
    which takes :class:`PottsModel2D`'s colours bit for bit).  The methods are :class:`PottsModel2D`'s; ``spins`` has shape (D, R, C).
    ``initial``: ``"random"`` (``default_rng(seed).integers(0, q, size)``) or one colour 0 .. q - 1 for every site.
    """

    _neighbours = 6

    def __init__(self, size, q, temperature: float = 1.0, coupling: float = 1.0, field=None, periodic=True,
                 seed: Optional[int] = None, initial="random", *, couplings=None, site_field=None):
        disordered = couplings is not None or site_field is not None
        if disordered:
            check_potts_temperature(q, temperature)
            self.field = None if field is None else np.array(field, dtype=np.float64)
        else:
            self.field = check_potts_model(q, coupling, field, temperature, 6)
        self.q = int(q)
        self.shape = (int(size),) * 3 if np.isscalar(size) else tuple(int(v) for v in size)
        if len(self.shape) != 3 or min(self.shape) < 1:
            raise ConfigurationError("size must be a positive edge or (depth, rows, cols)")
        self.depth, self.rows, self.cols = self.shape
        try:
            self.periodic = _hip.periodic_axes(periodic)
        except ValueError as e:
            raise ConfigurationError(str(e)) from None
        if any(p and n % 2 for p, n in zip(self.periodic, self.shape)):
            raise ConfigurationError("a periodic axis needs an even length")
        self.n_spins = self.depth * self.rows * self.cols
        if self.n_spins >= 2 ** 31:
            raise ConfigurationError("the lattice must hold fewer than 2^31 sites")
        if not (initial == "random" or (not isinstance(initial, (str, bool)) and int(initial) == initial and 0 <= int(initial) < self.q)):
            raise ConfigurationError(f"initial must be 'random' or a colour in 0 .. {self.q - 1}")
        self.coupling = float(coupling)
        self.temperature = float(temperature)
        self.seed = int(seed) if seed is not None else int(np.random.default_rng().integers(0, 2 ** 63))
        self.sweep_count = 0
        self.cluster_count = 0
        if disordered:
            self._open_disorder(couplings, site_field)
        else:
            self._lat = _hip.PottsLattice3D(self.depth, self.rows, self.cols, self.q, self.periodic)
            self._lat.set_model(self.coupling, self.field)
        if initial == "random":
            self._lat.set_spins(np.random.default_rng(self.seed).integers(0, self.q, size=self.shape).astype(np.int8))
        else:
            self._lat.fill(int(initial))


def potts_order_parameter(counts, q: int):
    """m = (q max_c N_c / N - 1) / (q - 1) from colour counts (last axis)."""
    counts = np.asarray(counts)
    return (q * counts.max(axis=-1) / counts.sum(axis=-1) - 1.0) / (q - 1.0)


def _scan(model_class, size, q, temperatures, coupling, n_equilibrate, n_measure, measure_every, algorithm, periodic, seed,
          couplings=None, site_field=None) -> dict:
    _algorithm(algorithm)
    disordered = couplings is not None or site_field is not None
    temperatures = [float(t) for t in temperatures]
    if int(n_measure) < 1 or int(measure_every) < 1 or int(n_equilibrate) < 0:
        raise ValueError("n_measure and measure_every must be >= 1, n_equilibrate >= 0")
    for t in temperatures:
        if disordered:
            check_potts_temperature(q, t)
        else:
            check_potts_model(q, coupling, None, t, model_class._neighbours)
    out = {k: [] for k in ("energy", "order_parameter", "specific_heat", "susceptibility", "binder")}
    for t in temperatures:
        model = model_class(size, q, temperature=t, coupling=coupling, periodic=periodic, seed=seed, couplings=couplings,
                            site_field=site_field)
        model.equilibrate(n_sweeps=int(n_equilibrate), algorithm=algorithm)
        rows = model.run(int(n_measure), int(measure_every), algorithm)
        N = model.n_spins
        model.close()
        if disordered:  # the stored couplings' own energy, summed on the device
            rows, E = rows
            e = E / N
        else:
            e = -float(coupling) * rows[:, 0] / N
        m = potts_order_parameter(rows[:, 1:], int(q))
        out["energy"].append(e.mean())
        out["order_parameter"].append(m.mean())
        out["specific_heat"].append(N * e.var() / t ** 2)
        out["susceptibility"].append(N * m.var() / t)
        m2 = np.mean(m ** 2)
        out["binder"].append(1.0 - np.mean(m ** 4) / (3.0 * m2 ** 2) if m2 > 0 else float("nan"))
    res = {k: np.array(v) for k, v in out.items()}
    res["temperatures"] = np.array(temperatures)
    return res


def potts_temperature_scan(size, q, temperatures, coupling: float = 1.0, n_equilibrate: int = 1000, n_measure: int = 50,
                           measure_every: int = 1, algorithm: str = "heat_bath", periodic: bool = True, seed: int = 0, *,
                           couplings=None, site_field=None) -> dict:
    """Per temperature: equilibrate a fresh lattice, then ``n_measure`` measurements ``measure_every`` updates apart, recorded on
    the device (tsu_potts2d_run).  Returns arrays over the temperatures: ``energy`` (per site), ``order_parameter``,
    ``specific_heat`` = N var(e) / T^2, ``susceptibility`` = N var(m) / T and the ``binder`` cumulant 1 - <m^4> / (3 <m^2>^2).
    ``couplings`` / ``site_field``: as for :class:`PottsModel2D`; the energy is then the stored couplings' (tsu_potts_dis_run)."""
    return _scan(PottsModel2D, size, q, temperatures, coupling, n_equilibrate, n_measure, measure_every, algorithm, periodic, seed,
                 couplings, site_field)


def potts_temperature_scan_3d(size, q, temperatures, coupling: float = 1.0, n_equilibrate: int = 1000, n_measure: int = 50,
                              measure_every: int = 1, algorithm: str = "heat_bath", periodic=True, seed: int = 0, *,
                              couplings=None, site_field=None) -> dict:
    """:func:`potts_temperature_scan` on the cubic lattice (:class:`PottsModel3D`, tsu_potts3d_run): the same keys."""
    return _scan(PottsModel3D, size, q, temperatures, coupling, n_equilibrate, n_measure, measure_every, algorithm, periodic, seed,
                 couplings, site_field)

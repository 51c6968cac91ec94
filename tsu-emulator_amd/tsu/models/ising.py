"""Ising models on the MI355X -- drop-in for the reference's ``tsu.models.ising``.

Same classes, signatures, return types and error messages as the reference (file:line cited per symbol).
What differs is where the work happens:

* :class:`IsingGrid` keeps the lattice as ``(rows, cols, J, h, periodic)`` and samples it with the hand-written
  red-black checkerboard HIP kernel (``libtsu_hip.so`` K1) on int8 spins.  The reference stores even a lattice
  as a dense N x N float64 matrix (ising.py:64,343-361) and walks it site by site; here ``.J`` is materialised
  lazily only when somebody reads it.  Checkerboard order is a different visiting order of the same heat-bath
  kernel: same stationary distribution, different trajectory.
* :class:`IsingModel` / :class:`IsingChain` (arbitrary graph) go through the dense HIP path of
  :class:`tsu.gibbs.GibbsSampler` in the reference's own sequential order.

``bias_mode``.  The reference's spin->bit bias conversion has a sign error (ising.py:148 returns
``-2h + 2 rowsum(J)``; the conversion of E = -1/2 s'Js - h's is ``+2h - 2 rowsum(J)``), so as shipped it samples
an Ising model with effective field ``h_eff = 2 rowsum(J) - h``.  ``bias_mode="compat"`` (default for the
reference-named classes, bug-for-bug drop-in) reproduces that; ``bias_mode="physical"`` uses the corrected
conversion (default of the README-named :class:`IsingModel2D`).

Quenched disorder (K7).  ``IsingModel2D(..., couplings=(J_right, J_down), field=h)`` keeps per-bond couplings and per-site
fields on the device (fp32, physical mode only) -- Edwards-Anderson spin glasses, random-field and Mattis magnets, Ising-prior
denoising -- and ``gibbs_update`` then runs the disordered heat-bath kernel with K1's own site uniforms and sweep counter.
``energy()`` is the disordered energy, ``overlap(other)`` the spin-glass overlap q / N, and ``temperature_scan(...,
couplings=, field=, replicas=2)`` adds <|q|>, <q^2> and the Binder ratio of two replicas per temperature.
:class:`LatticeTempering` / :func:`tempering_scan` run such a scan as replica exchange: ladders of walkers on one disorder, swept
in batches and swapped between temperatures on the device; :class:`LatticeTempering3D` / :func:`tempering_scan_3d` do the same
for the cubic lattices of :class:`IsingModel3D` (K8).
"""
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from .. import _hip
from ..gibbs import GibbsConfig, GibbsSampler, _content_key


@dataclass
class IsingConfig:
    """Reference: tsu/models/ising.py:25-36."""

    temperature: float = 1.0
    external_field: float = 0.0  # uniform external field h
    n_burnin: int = 100
    n_sweeps: int = 10

    def __post_init__(self):
        if self.temperature <= 0:
            raise ValueError("Temperature must be positive")


def _mode_id(bias_mode: str) -> int:
    if bias_mode not in ("compat", "physical"):
        raise ValueError("bias_mode must be 'compat' or 'physical'")
    return _hip.MODE_COMPAT if bias_mode == "compat" else _hip.MODE_PHYSICAL


class IsingModel:
    """General Ising model on an arbitrary graph.  Reference: tsu/models/ising.py:39-262.

    ``graph="dense"`` keeps the coupling matrix as the reference does (an N x N array, sites visited in raster order on
    the dense kernel K2).  ``graph="sparse"`` keeps only the couplings that were set (``scipy.sparse``) and samples on
    the colour-parallel sparse kernel K5 -- the sequential loop of gibbs.py:128-162 in the colour-major visiting order of
    a proper colouring -- which is what makes a 10^6-site chain possible (its dense J would be 8 TB).  ``"auto"``
    (default): sparse above ``DENSE_LIMIT`` sites, dense below."""

    DENSE_LIMIT = 16384  # largest N for which a dense J is kept / may be materialised (2 GiB of float64)

    def __init__(self, n_spins: int, config: Optional[IsingConfig] = None, *, bias_mode: str = "compat", graph: str = "auto"):
        _mode_id(bias_mode)
        if graph not in ("auto", "dense", "sparse"):
            raise ValueError("graph must be 'auto', 'dense' or 'sparse'")
        self.n_spins = n_spins
        self.config = config or IsingConfig()
        self.bias_mode = bias_mode
        self.sparse = graph == "sparse" or (graph == "auto" and n_spins > self.DENSE_LIMIT)
        if self.sparse:
            import scipy.sparse as sp
            self._J = None
            self._Jsp = sp.csr_matrix((n_spins, n_spins), dtype=np.float64)
        else:
            self._J = np.zeros((n_spins, n_spins))
        self.h = np.ones(n_spins) * self.config.external_field
        gibbs_config = GibbsConfig(temperature=self.config.temperature, n_burnin=self.config.n_burnin,
                                   n_sweeps=self.config.n_sweeps)
        self.sampler = GibbsSampler(gibbs_config)

    # ``J`` is a plain attribute in the reference; a property here so that IsingGrid can build it lazily
    @property
    def J(self) -> np.ndarray:
        if getattr(self, "sparse", False):
            if self.n_spins > self.DENSE_LIMIT:
                raise MemoryError(f"dense J for {self.n_spins} spins would need {8 * self.n_spins ** 2 / 2 ** 30:.0f} GiB; "
                                  "the sparse kernel does not need it (see .J_sparse)")
            dense = self._Jsp.toarray()
            dense.setflags(write=False)  # a copy: edits would be lost -- use set_coupling()
            return dense
        return self._J

    @J.setter
    def J(self, value):
        if getattr(self, "sparse", False):
            import scipy.sparse as sp
            self._Jsp = sp.csr_matrix(value, dtype=np.float64)
            self.sampler.invalidate()
        else:
            self._J = np.asarray(value, dtype=float)

    @property
    def J_sparse(self):
        """The coupling matrix as ``scipy.sparse`` CSR (sparse models: the stored graph; dense models: a conversion)."""
        import scipy.sparse as sp
        return self._csr() if self.sparse else sp.csr_matrix(self.J)

    def _csr(self):
        """CSR form of a sparse model's couplings (converted once after the last set_coupling: energy() runs per sample)."""
        if getattr(self._Jsp, "format", "") != "csr":
            self._Jsp = self._Jsp.tocsr()
        return self._Jsp

    def set_coupling(self, i: int, j: int, strength: float):
        """Reference: ising.py:77-86 (symmetric assignment, not accumulation)."""
        if self.sparse:
            if not hasattr(self._Jsp, "rows"):       # CSR -> LIL once: cheap element assignment
                self._Jsp = self._Jsp.tolil()
            self._Jsp[i, j] = strength
            self._Jsp[j, i] = strength
        else:
            self.J[i, j] = strength
            self.J[j, i] = strength
        self.sampler.invalidate()

    def set_external_field(self, field: np.ndarray):
        """Reference: ising.py:88-97."""
        if len(field) != self.n_spins:
            raise ValueError(f"Field must have length {self.n_spins}")
        self.h = np.array(field)

    def energy(self, state: np.ndarray) -> float:
        """Reference: ising.py:99-117 -- E(s) = -1/2 s'Js - h's."""
        state = np.asarray(state)
        if self.sparse:
            interaction_energy = -0.5 * state.dot(self._csr().dot(state))
        else:
            interaction_energy = -0.5 * state.dot(self.J).dot(state)
        field_energy = -self.h.dot(state)
        return interaction_energy + field_energy

    def _spins_to_bits(self, spins: np.ndarray) -> np.ndarray:
        """Reference: ising.py:119-121."""
        return ((spins + 1) // 2).astype(int)

    def _bits_to_spins(self, bits: np.ndarray) -> np.ndarray:
        """Reference: ising.py:123-125."""
        return 2 * bits - 1

    def _get_bit_coupling(self) -> np.ndarray:
        """Reference: ising.py:127-138 -- J_bit = 4 J."""
        if self.sparse:
            return (4 * self._csr()).tocsr()
        return 4 * self.J

    def _get_bit_bias(self) -> np.ndarray:
        """Reference: ising.py:140-148 (``compat``: verbatim, including its sign), or the corrected conversion."""
        rowsum = np.asarray(self._csr().sum(axis=1)).ravel() if self.sparse else np.sum(self.J, axis=1)
        if self.bias_mode == "compat":
            return -2 * self.h + 2 * rowsum
        return 2 * self.h - 2 * rowsum

    def sample(self, n_samples: int = 1000, initial_state: Optional[np.ndarray] = None) -> np.ndarray:
        """Reference: ising.py:150-181 -- (n_samples, n_spins) array of +-1."""
        J_bit = self._get_bit_coupling()
        h_bit = self._get_bit_bias()
        initial_bits = self._spins_to_bits(np.asarray(initial_state)) if initial_state is not None else None
        bit_samples = self.sampler.sample_boltzmann(J_bit, bias=h_bit, n_samples=n_samples, initial_state=initial_bits)
        return self._bits_to_spins(bit_samples)

    def magnetization(self, samples: np.ndarray) -> float:
        """Reference: ising.py:183-193."""
        return np.mean(np.sum(samples, axis=1)) / self.n_spins

    def specific_heat(self, samples: np.ndarray) -> float:
        """Reference: ising.py:195-213."""
        energies = np.array([self.energy(s) for s in samples])
        mean_E = np.mean(energies)
        mean_E2 = np.mean(energies ** 2)
        T = self.config.temperature
        return float((mean_E2 - mean_E ** 2) / (T ** 2 * self.n_spins))

    def susceptibility(self, samples: np.ndarray) -> float:
        """Reference: ising.py:215-233."""
        magnetizations = np.sum(samples, axis=1) / self.n_spins
        mean_M = np.mean(magnetizations)
        mean_M2 = np.mean(magnetizations ** 2)
        T = self.config.temperature
        return (mean_M2 - mean_M ** 2) * self.n_spins / T

    def find_ground_state(self, n_steps: int = 1000) -> Tuple[np.ndarray, float]:
        """Reference: ising.py:235-262 (simulated annealing from 10 T down to 0.01 T)."""
        J_bit = self._get_bit_coupling()
        h_bit = self._get_bit_bias()
        best_bits, _ = self.sampler.simulated_annealing(J_bit, bias=h_bit, T_initial=10.0 * self.config.temperature,
                                                        T_final=0.01 * self.config.temperature, n_steps=n_steps)
        ground_state = self._bits_to_spins(best_bits)
        return ground_state, self.energy(ground_state)


class IsingChain(IsingModel):
    """1-D chain with open ends.  Reference: ising.py:265-304."""

    def __init__(self, n_spins: int, J: float = 1.0, config: Optional[IsingConfig] = None, *, bias_mode: str = "compat",
                 graph: str = "auto"):
        super().__init__(n_spins, config, bias_mode=bias_mode, graph=graph)
        if self.sparse:
            import scipy.sparse as sp
            off = np.full(max(n_spins - 1, 0), float(J))
            self._Jsp = sp.diags([off, off], [1, -1], shape=(n_spins, n_spins), format="csr", dtype=np.float64)
        else:
            for i in range(n_spins - 1):
                self._J[i, i + 1] = J
                self._J[i + 1, i] = J

    def visualize(self, state: np.ndarray, title: str = "Ising Chain"):
        """Reference: ising.py:288-304."""
        import matplotlib.pyplot as plt
        plt.figure(figsize=(12, 2))
        colors = ["blue" if s == 1 else "red" for s in state]
        plt.bar(range(self.n_spins), np.ones(self.n_spins), color=colors, width=1.0)
        plt.xlabel("Spin Index")
        plt.ylabel("State")
        plt.title(title)
        plt.ylim([0, 1.2])
        plt.tight_layout()
        return plt.gcf()


def _grid_coupling(rows: int, cols: int, J: float, periodic: bool) -> np.ndarray:
    """Dense coupling matrix of the square lattice, bond by bond as ising.py:343-361 builds it (bonds are SET:
    on a periodic dimension of size 2 the wrap bond coincides with the direct one, of size 1 it is J_ii)."""
    n = rows * cols
    M = np.zeros((n, n))
    for i in range(rows):
        for j in range(cols):
            idx = i * cols + j
            if j < cols - 1:
                M[idx, idx + 1] = M[idx + 1, idx] = J
            elif periodic:
                M[idx, i * cols] = M[i * cols, idx] = J
            if i < rows - 1:
                M[idx, idx + cols] = M[idx + cols, idx] = J
            elif periodic:
                M[idx, j] = M[j, idx] = J
    return M


class IsingGrid(IsingModel):
    """2-D square lattice, nearest neighbours.  Reference: ising.py:307-421.

    Sampling runs on the lattice kernel whenever the model is still the uniform lattice it was built as
    (no ``set_coupling`` edits, uniform field) and the checkerboard exists (open boundaries: any shape;
    periodic: even dimensions >= 4).  Otherwise it falls through to the dense path of :class:`IsingModel`
    on the materialised matrix -- still on the GPU, in the reference's raster order.
    """

    DENSE_LIMIT = 16384  # largest N for which .J may be materialised (2 GiB of float64)

    def __init__(self, size: Tuple[int, int], J: float = 1.0, config: Optional[IsingConfig] = None,
                 periodic: bool = False, *, bias_mode: str = "compat", seed: Optional[int] = None):
        _mode_id(bias_mode)
        self.rows, self.cols = size
        self.n_spins = self.rows * self.cols
        self.config = config or IsingConfig()
        self.bias_mode = bias_mode
        self.periodic = periodic
        self.coupling = float(J)
        self.sparse = False     # the lattice has its own kernel (K1); the dense view is built on first access
        self._J = None
        self._custom = False    # set_coupling() was called / J was edited: no longer a uniform lattice
        self._J_key = None
        self.h = np.ones(self.n_spins) * self.config.external_field
        gibbs_config = GibbsConfig(temperature=self.config.temperature, n_burnin=self.config.n_burnin,
                                   n_sweeps=self.config.n_sweeps)
        self.sampler = GibbsSampler(gibbs_config)
        self._seed = None if seed is None else int(seed)
        self._sweep_counter = 0
        self._lattice = None

    # ------------------------------------------------------------------ dense view (lazy)
    @property
    def J(self) -> np.ndarray:
        if self._J is None:
            if self.n_spins > self.DENSE_LIMIT:
                raise MemoryError(f"dense J for {self.n_spins} spins would need {8 * self.n_spins ** 2 / 2 ** 30:.0f} GiB; "
                                  "the lattice kernel does not need it")
            self._J = _grid_coupling(self.rows, self.cols, self.coupling, self.periodic)
            self._J_key = _content_key(self._J)
        return self._J

    @J.setter
    def J(self, value):
        self._J = np.asarray(value, dtype=float)
        self._custom = True

    def _J_edited_in_place(self) -> bool:
        """The reference lets callers write into ``grid.J`` and samples from whatever it holds (ising.py:150-181 reads
        ``self.J`` at call time).  Once the dense matrix has been handed out, every sampling call therefore checks
        (full content hash) that it still is the uniform lattice before taking the lattice kernel."""
        if self._J is None or self._custom:
            return False
        if _content_key(self._J) != self._J_key:
            self._custom = True
            return True
        return False

    def set_coupling(self, i: int, j: int, strength: float):
        super().set_coupling(i, j, strength)
        self._custom = True

    # ------------------------------------------------------------------ lattice kernel plumbing
    def _lattice_ok(self) -> bool:
        if self._custom or self._J_edited_in_place() or np.any(self.h != self.h[0]):
            return False
        if self.periodic and (self.rows % 2 or self.cols % 2 or self.rows < 4 or self.cols < 4):
            return False  # no 2-colouring (and the reference's size-1/2 wrap bonds are special): dense path
        return True

    def _philox_seed(self) -> int:
        if self._seed is None:
            self._seed = int(np.random.randint(0, 2 ** 31 - 1)) | (int(np.random.randint(0, 2 ** 31 - 1)) << 31)
        return self._seed

    def _device_lattice(self) -> "_hip.Lattice":
        if self._lattice is None:
            self._lattice = _hip.Lattice(self.rows, self.cols, self.periodic)
        return self._lattice

    def _set_model(self, lat):
        # temperature is read at call time from the sampler's config, which callers mutate in place
        # (ising.py:491-492, gibbs.py:382)
        lat.set_model(self.coupling, float(self.h[0]), float(self.sampler.config.temperature), _mode_id(self.bias_mode))

    def _flat_to_grid(self, flat_state: np.ndarray) -> np.ndarray:
        """Reference: ising.py:363-365."""
        return flat_state.reshape(self.rows, self.cols)

    def _grid_to_flat(self, grid_state: np.ndarray) -> np.ndarray:
        """Reference: ising.py:367-369."""
        return grid_state.flatten()

    # ------------------------------------------------------------------ sampling / observables
    def sample(self, n_samples: int = 1000, initial_state: Optional[np.ndarray] = None) -> np.ndarray:
        """Reference: ising.py:150-181 specialised to the lattice: burn-in, then ``n_samples`` x ``n_sweeps``
        checkerboard sweeps, recording the lattice after each.  Returns (n_samples, N) int array of +-1."""
        if not self._lattice_ok():
            return super().sample(n_samples, initial_state)
        lat = self._device_lattice()
        cfg = self.sampler.config
        if initial_state is not None:
            s0 = np.asarray(initial_state).reshape(self.rows, self.cols)
            if not np.all((s0 == 1) | (s0 == -1)):
                raise ValueError("initial_state must contain only +1 / -1")
            lat.set_spins(s0.astype(np.int8))
        else:
            bits = np.random.randint(0, 2, size=self.n_spins)  # the reference's draw (gibbs.py:201)
            lat.set_spins((2 * bits - 1).astype(np.int8).reshape(self.rows, self.cols))
        self._set_model(lat)
        seed = self._philox_seed()
        samples = np.zeros((n_samples, self.n_spins), dtype=int)
        # burn-in and the n_samples x n_sweeps loop in as few device calls as a 1 GiB staging buffer allows
        chunk = max(1, min(int(n_samples), (1 << 30) // max(1, self.n_spins)))
        done, burn = 0, int(cfg.n_burnin)
        if n_samples == 0:
            lat.sweep(burn, seed, self._sweep_counter)
            self._sweep_counter += burn
        while done < n_samples:
            m = min(chunk, n_samples - done)
            samples[done:done + m] = lat.sample(burn, int(cfg.n_sweeps), m, seed, self._sweep_counter).reshape(m, -1)
            self._sweep_counter += burn + m * int(cfg.n_sweeps)
            self.sampler.sample_count += m
            done += m
            burn = 0
        return samples

    def energy(self, state: np.ndarray) -> float:
        """Reference: ising.py:99-117; on the lattice path E = -J sum_bonds s_i s_j - h sum_i s_i by a device
        reduction (no dense matrix)."""
        state = np.asarray(state)
        if not self._lattice_ok():
            return super().energy(state.reshape(-1))
        lat = self._device_lattice()
        lat.set_spins(state.reshape(self.rows, self.cols).astype(np.int8))
        sum_s, sum_bonds = lat.observables()
        return -self.coupling * float(sum_bonds) - float(self.h[0]) * float(sum_s)

    def visualize(self, state: np.ndarray, title: str = "Ising Grid", cmap: str = "RdBu_r"):
        """Reference: ising.py:371-401."""
        import matplotlib.pyplot as plt
        if state.ndim == 1:
            state = self._flat_to_grid(state)
        fig, ax = plt.subplots(figsize=(8, 8))
        im = ax.imshow(state, cmap=cmap, vmin=-1, vmax=1, interpolation="nearest")
        ax.set_title(title, fontsize=14, fontweight="bold")
        ax.set_xlabel("Column Index")
        ax.set_ylabel("Row Index")
        cbar = plt.colorbar(im, ax=ax, fraction=0.046, pad=0.04)
        cbar.set_label("Spin State", rotation=270, labelpad=20)
        cbar.set_ticks([-1, 0, 1])
        cbar.set_ticklabels(["-1", "0", "+1"])
        plt.tight_layout()
        return fig

    def compute_domains(self, state: np.ndarray) -> int:
        """Reference: ising.py:403-421 (boundary count // 2 + 1; open-boundary differences only)."""
        if state.ndim == 1:
            state = self._flat_to_grid(state)
        horizontal_boundaries = np.sum(state[:, :-1] != state[:, 1:])
        vertical_boundaries = np.sum(state[:-1, :] != state[1:, :])
        return (horizontal_boundaries + vertical_boundaries) // 2 + 1


_ALGORITHMS = ("gibbs", "swendsen_wang", "swendsen_wang_ghost")


def _check_algorithm(algorithm: str) -> None:
    if algorithm not in _ALGORITHMS:
        raise ValueError(f"algorithm must be one of {_ALGORITHMS}, got {algorithm!r}")


def _refuse_ghost_2d() -> None:
    """The ghost-spin steps live on the 3-D handle; a one-layer lattice there is the 2-D model."""
    raise _hip.UnsupportedError("ghost-spin Swendsen-Wang steps (algorithm='swendsen_wang_ghost') run on the 3-D lattice handle: "
                                "use IsingModel3D(size=(1, R, C), periodic=(False, p, p)) for an R x C lattice in a field")


def _check_cluster_model(external_field: float, bias_mode: str) -> None:
    """Swendsen-Wang samples the physical zero-field measure: refuse anything else before the device is touched."""
    if external_field != 0:
        raise _hip.UnsupportedError("Swendsen-Wang cluster updates need external_field == 0 (a field would need a ghost spin)")
    if bias_mode != "physical":
        raise _hip.UnsupportedError("Swendsen-Wang cluster updates need bias_mode='physical' (compat mode's bias is not the "
                                    "zero-field Ising measure)")


def _set_cluster_measure(model, on: bool) -> None:
    """Flip the handle's cluster-size record switch only when it changes (a host-side flag: no launch, no allocation)."""
    if bool(on) != model._measuring:
        model._lat.cluster_measure(bool(on))
        model._measuring = bool(on)


def _check_improved(improved: bool, algorithm: str) -> None:
    if improved and algorithm == "gibbs":
        raise _hip.UnsupportedError("improved=True needs the cluster decomposition of a Swendsen-Wang step: use "
                                    "algorithm='swendsen_wang' (or 'swendsen_wang_ghost' on a 3-D lattice in a field)")


def cluster_estimators(record: dict) -> dict:
    """Improved estimators per step from a model's ``cluster_record()`` dict, float64 arrays from the exact integers (N is the
    record's ``n_spins``):

    ``m2`` = (sum_m2 + m_frozen^2) / N^2, whose mean is <M^2> / N^2 (the free clusters' signs average out given the bonds; the
    frozen sites keep theirs); ``m4`` = (3 sum_m2^2 - 2 sum_m4) / N^4, whose mean is <M^4> / N^4 at zero field (NaN on a step
    with frozen sites), computed in Python integers before the one division; ``m`` = m_frozen / N, whose mean is <M> / N with a
    ghost spin (0 at zero field); ``mean_cluster_size`` = sum_size2 / N, the FK mean size of the free cluster of a site."""
    N = int(record["n_spins"])
    s2 = [int(v) for v in record["sum_m2"]]
    s4 = [int(v) for v in record["sum_m4"]]
    mf = [int(v) for v in record["m_frozen"]]
    nf = [int(v) for v in record["n_frozen"]]
    return {
        "m2": np.array([(a + f * f) / N ** 2 for a, f in zip(s2, mf)], dtype=np.float64),
        "m4": np.array([(3 * a * a - 2 * b) / N ** 4 if k == 0 else np.nan for a, b, k in zip(s2, s4, nf)], dtype=np.float64),
        "m": np.array([f / N for f in mf], dtype=np.float64),
        "mean_cluster_size": np.array([int(v) / N for v in record["sum_size2"]], dtype=np.float64),
    }


def _disorder_arrays(rows: int, cols: int, periodic: bool, coupling: float, external_field: float, bias_mode: str,
                     couplings, field):
    """Validate K7 disorder (before any device call) and round it once to fp32: (J_right, J_down, h or None)."""
    if bias_mode != "physical":
        raise ValueError("couplings / field arrays need bias_mode='physical'")
    if couplings is not None and coupling != 1.0:
        raise ValueError("give either couplings=(J_right, J_down) or a scalar coupling, not both")
    if field is not None and external_field != 0.0:
        raise ValueError("give either field= or a non-zero external_field, not both")
    shape = (rows, cols)

    def arr(a, name):
        a = np.asarray(a, dtype=np.float64)
        if a.shape != shape:
            raise ValueError(f"{name} must have shape {shape}, got {a.shape}")
        if not np.all(np.isfinite(a)):
            raise ValueError(f"{name} must be finite")
        with np.errstate(over="ignore"):
            a32 = a.astype(np.float32)
        if not np.all(np.isfinite(a32)):
            raise ValueError(f"{name} overflows float32")
        return a32

    if couplings is not None:
        if len(couplings) != 2:
            raise ValueError("couplings must be a pair (J_right, J_down)")
        jr, jd = arr(couplings[0], "J_right"), arr(couplings[1], "J_down")
    else:
        jr = np.full(shape, coupling, dtype=np.float32)
        jd = np.full(shape, coupling, dtype=np.float32)
        if not periodic:
            jr[:, -1] = 0.0
            jd[-1, :] = 0.0
    if not periodic and (np.any(jr[:, -1] != 0) or np.any(jd[-1, :] != 0)):
        raise ValueError("open lattice: the last column of J_right and the last row of J_down must be 0")
    if field is not None:
        h = arr(field, "field")
    else:
        h = np.full(shape, external_field, dtype=np.float32) if external_field != 0.0 else None
    return jr, jd, h


# ---------------------------------------------------------------- correlation length: k_min modes of the axis profiles
def _kmin_tables(L: int):
    """(cos, sin) of 2 pi x / L for x = 0 .. L - 1 in float64: the tables the host hands to the device."""
    ang = 2.0 * np.pi * np.arange(int(L), dtype=np.float64) / float(L)
    return np.cos(ang), np.sin(ang)


def _ordered_sum(terms: np.ndarray) -> float:
    """The sum of float64 terms in the order of the device's mode pass (csrc/corr_dev.h): partial t of 256 adds the terms t, t + 256,
    ... in ascending order from 0.0; the 64 partials of each of the four groups fold by halves (32, 16, .., 1); (g0 + g1) + (g2 + g3)."""
    acc = np.zeros(256)
    for lo in range(0, terms.size, 256):
        chunk = terms[lo:lo + 256]
        acc[:chunk.size] += chunk
    w = acc.reshape(4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w[:, :off] + w[:, off:2 * off]
    return float((w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0]))


def _kmin_modes(profiles, periodic) -> np.ndarray:
    """complex128 F_d = sum_x P_d[x] (cos(2 pi x / L_d) + i sin(2 pi x / L_d)) per axis, NaN on an open axis."""
    out = np.full(len(profiles), complex(np.nan, np.nan), dtype=np.complex128)
    for d, (P, per) in enumerate(zip(profiles, periodic)):
        if per:
            c, sn = _kmin_tables(len(P))
            Pf = np.asarray(P, dtype=np.int64).astype(np.float64)
            out[d] = complex(_ordered_sum(Pf * c), _ordered_sum(Pf * sn))
    return out


def _check_correlation(periodic) -> None:
    if not any(periodic):
        raise ValueError("correlation=True needs at least one periodic axis (no k_min mode is defined on an open axis)")


def correlation_length(f2, F2, lengths) -> np.ndarray:
    """xi_d = sqrt(<f_tot^2> / <|F_d|^2> - 1) / (2 sin(pi / L_d)) per axis (last index of F2); NaN where the radicand is negative
    or the axis has no mode."""
    f2 = np.asarray(f2, dtype=np.float64)[..., None]
    F2 = np.asarray(F2, dtype=np.float64)
    L = np.asarray(lengths, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rad = f2 / F2 - 1.0
        return np.where(rad >= 0, np.sqrt(np.where(rad >= 0, rad, 0.0)), np.nan) / (2.0 * np.sin(np.pi / L))


def _correlation_summary(out: dict, N: int, lengths, periodic, f2, F2) -> dict:
    """chi_k, xi and xi_over_L from <f_tot^2> (n_T,) and <|F_d|^2> (n_T, n_axes; NaN on open axes)."""
    per = np.asarray(periodic, dtype=bool)
    out["chi_k"] = np.asarray(F2, dtype=np.float64) / N
    out["xi"] = correlation_length(f2, F2, lengths)
    out["xi_over_L"] = np.mean(out["xi"][:, per] / np.asarray(lengths, dtype=np.float64)[per], axis=1)
    return out


def lattice_bond_count(shape, periodic) -> int:
    """N_b: the bonds of the lattice's energy, every site's bond along each axis, the last one of an open axis dropped and the wrap
    bond of a periodic axis kept (a periodic axis of length 1 or 2 counts its wrap bond as the energy does)."""
    shape = tuple(int(n) for n in shape)
    per = (bool(periodic),) * len(shape) if isinstance(periodic, (bool, np.bool_)) else tuple(bool(p) for p in periodic)
    N = int(np.prod(shape))
    return sum(N if p else N - N // n for n, p in zip(shape, per))


class IsingModel2D:
    """README facade (README.md:116-131): a lattice that lives on the GPU between calls.

    ``IsingModel2D(size=50, coupling=1.0, temperature=2.5)``; ``gibbs_update()`` = one checkerboard sweep;
    ``cluster_update()`` = one Swendsen-Wang step (zero field, physical mode; its own counter ``cluster_count``);
    ``magnetization()`` / ``energy()`` = observables of the current state by a device reduction;
    ``equilibrate(T)`` sets the temperature, runs ``n_sweeps`` sweeps (or SW steps) and returns ``self``.

    ``couplings=(J_right, J_down)`` and ``field`` (``(rows, cols)`` arrays, physical mode) make the lattice disordered (K7):
    ``J_right[r, c]`` couples (r, c) to (r, c+1), ``J_down[r, c]`` couples (r, c) to (r+1, c) (both wrap on a periodic
    lattice; on an open one the last column / row must be 0), ``field[r, c]`` is the field of site (r, c).  The arrays are
    rounded once to float32 (``disorder`` returns the rounded copies).  ``set_disorder`` replaces them and keeps the spins
    and counters, ``clear_disorder`` returns to the uniform model.  Cluster updates refuse a disordered lattice.
    """

    _disorder = None  # (J_right, J_down, h or None) float32 while the lattice is disordered

    def __init__(self, size, coupling: float = 1.0, temperature: float = 1.0, periodic: bool = True,
                 external_field: float = 0.0, seed: Optional[int] = None, bias_mode: str = "physical",
                 initial: str = "random", *, couplings=None, field=None):
        if temperature <= 0:
            raise ValueError("Temperature must be positive")
        self.rows, self.cols = (size, size) if np.isscalar(size) else tuple(size)
        self.n_spins = self.rows * self.cols
        self.coupling = float(coupling)
        self.temperature = float(temperature)
        self.external_field = float(external_field)
        self.periodic = bool(periodic)
        self.bias_mode = bias_mode
        self._mode = _mode_id(bias_mode)
        if initial not in ("random", "up", "down"):
            raise ValueError("initial must be 'random', 'up' or 'down'")
        self._disorder = None
        if couplings is not None or field is not None:
            self._disorder = _disorder_arrays(self.rows, self.cols, self.periodic, self.coupling, self.external_field,
                                              bias_mode, couplings, field)
        self.seed = int(seed) if seed is not None else (
            int(np.random.randint(0, 2 ** 31 - 1)) | (int(np.random.randint(0, 2 ** 31 - 1)) << 31))
        self.sweep_count = 0
        self.cluster_count = 0
        self._measuring = False  # the handle's cluster-size record switch
        self._lat = _hip.Lattice(self.rows, self.cols, self.periodic)
        if initial == "random":
            self._lat.randomize(self.seed)
        elif initial in ("up", "down"):
            self._lat.fill(1 if initial == "up" else -1)
        if self._disorder is not None:
            self._lat.set_disorder(*self._disorder)

    @property
    def disorder(self):
        """(J_right, J_down, h or None) as stored on the device (float32), or None for the uniform model."""
        if self._disorder is None:
            return None
        return tuple(None if a is None else a.copy() for a in self._disorder)

    def set_disorder(self, couplings=None, field=None) -> "IsingModel2D":
        """Replace the quenched disorder (``couplings=None``: uniform ``coupling``; ``field=None``: ``external_field``);
        the spins and counters are kept."""
        d = _disorder_arrays(self.rows, self.cols, self.periodic, self.coupling, self.external_field, self.bias_mode,
                             couplings, field)
        self._lat.set_disorder(*d)
        self._disorder = d
        return self

    def clear_disorder(self) -> "IsingModel2D":
        """Back to the uniform model (K1 sweeps, same seed and sweep counter)."""
        self._lat.clear_disorder()
        self._disorder = None
        return self

    def gibbs_update(self, n_sweeps: int = 1) -> "IsingModel2D":
        if self._disorder is not None:
            self._lat.disorder_sweep(self.temperature, int(n_sweeps), self.seed, self.sweep_count)
        else:
            self._lat.set_model(self.coupling, self.external_field, self.temperature, self._mode)
            self._lat.sweep(int(n_sweeps), self.seed, self.sweep_count)
        self.sweep_count += int(n_sweeps)
        return self

    def cluster_update(self, n_steps: int = 1, measure: bool = False) -> "IsingModel2D":
        """n_steps Swendsen-Wang steps (K6); the heat-bath stream and ``sweep_count`` are not touched.  ``measure=True``: the same
        spins, and one cluster-size row per step for :meth:`cluster_record`."""
        if self._disorder is not None:
            raise _hip.UnsupportedError("Swendsen-Wang cluster updates do not take a disordered lattice (couplings / field)")
        _check_cluster_model(self.external_field, self.bias_mode)
        _set_cluster_measure(self, measure)
        self._lat.cluster_sweep(self.coupling, self.temperature, int(n_steps), self.seed, self.cluster_count)
        self.cluster_count += int(n_steps)
        return self

    def cluster_record(self) -> dict:
        """The cluster-size record of the last measured call (``cluster_update(measure=True)`` or a scan with ``improved=True``):
        arrays over its steps, exact integers from the device: ``n_clusters``, ``largest``, ``sum_size2``, ``sum_m2`` (int64),
        ``sum_m4`` (Python ints, it passes 2^64), ``n_frozen``, ``m_frozen`` (0 at zero field), and ``n_spins``.  Feed it to
        :func:`cluster_estimators`."""
        rec = self._lat.cluster_record()
        rec["n_spins"] = self.n_spins
        return rec

    def equilibrate(self, temperature: Optional[float] = None, n_sweeps: int = 1000,
                    algorithm: str = "gibbs") -> "IsingModel2D":
        _check_algorithm(algorithm)
        if algorithm == "swendsen_wang_ghost":
            _refuse_ghost_2d()
        if temperature is not None:
            if temperature <= 0:
                raise ValueError("Temperature must be positive")
            self.temperature = float(temperature)
        if algorithm == "swendsen_wang":
            return self.cluster_update(n_sweeps)
        return self.gibbs_update(n_sweeps)

    def magnetization(self) -> float:
        sum_s, _ = self._lat.observables()
        return sum_s / self.n_spins

    def energy(self) -> float:
        if self._disorder is not None:
            return self._lat.disorder_energy()
        sum_s, sum_bonds = self._lat.observables()
        return -self.coupling * float(sum_bonds) - self.external_field * float(sum_s)

    def overlap(self, other: "IsingModel2D") -> float:
        """q / N = sum_i s_i s'_i / N with another model of the same shape (a device reduction)."""
        if (other.rows, other.cols) != (self.rows, self.cols):
            raise ValueError(f"overlap needs equal shapes, got {(self.rows, self.cols)} and {(other.rows, other.cols)}")
        return self._lat.overlap(other._lat) / self.n_spins

    def link_overlap(self, other: "IsingModel2D") -> float:
        """q_l = L / N_b with another model of the same shape and boundary: L = sum over the energy's bonds (i, j) of
        s_i s'_i s_j s'_j (an exact integer, a device reduction), N_b the number of those bonds."""
        if (other.rows, other.cols) != (self.rows, self.cols) or other.periodic != self.periodic:
            raise ValueError(f"link_overlap needs equal shapes and boundaries, got {(self.rows, self.cols)} and {(other.rows, other.cols)}")
        L, nb = self._lat.link_overlap(other._lat)
        return L / nb

    def axis_profiles(self, other: Optional["IsingModel2D"] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(P_row, P_col): exact int64 sums of the spins (of s s' with ``other``) over the columns / the rows, on the device."""
        if other is not None and (other.rows, other.cols) != (self.rows, self.cols):
            raise ValueError(f"axis_profiles needs equal shapes, got {(self.rows, self.cols)} and {(other.rows, other.cols)}")
        return self._lat.profiles(None if other is None else other._lat)

    def fourier_modes(self, other: Optional["IsingModel2D"] = None) -> np.ndarray:
        """complex128 (2,): the k_min = 2 pi / L modes of the row and the column profile (NaN on an open lattice), summed on the
        host from the device's profiles in the fixed order of the ladders' mode pass."""
        return _kmin_modes(self.axis_profiles(other), (self.periodic, self.periodic))

    @property
    def spins(self) -> np.ndarray:
        return self._lat.get_spins()

    @spins.setter
    def spins(self, value):
        v = np.asarray(value).reshape(self.rows, self.cols)
        if not np.all((v == 1) | (v == -1)):
            raise ValueError("spins must be +1 / -1")
        self._lat.set_spins(v.astype(np.int8))


def demonstrate_phase_transition(sizes: List[int] = [8, 16, 32], temperatures: Optional[np.ndarray] = None) -> dict:
    """Reference: ising.py:424-476 -- |M|, chi and C over a temperature scan for several lattice sizes."""
    if temperatures is None:
        temperatures = np.linspace(0.5, 4.0, 15)
    results = {}
    for size in sizes:
        print(f"\nSimulating {size}×{size} Ising grid...")
        magnetizations, susceptibilities, specific_heats = [], [], []
        for T in temperatures:
            model = IsingGrid((size, size), J=1.0, config=IsingConfig(temperature=T, n_burnin=200, n_sweeps=10))
            samples = model.sample(n_samples=500)
            mag = abs(model.magnetization(samples))
            chi = model.susceptibility(samples)
            C = model.specific_heat(samples)
            magnetizations.append(mag)
            susceptibilities.append(chi)
            specific_heats.append(C)
            print(f"  T={T:.2f}: |M|={mag:.3f}, χ={chi:.3f}, C={C:.3f}")
        results[size] = {
            "temperatures": temperatures,
            "magnetizations": np.array(magnetizations),
            "susceptibilities": np.array(susceptibilities),
            "specific_heats": np.array(specific_heats),
        }
    return results


def temperature_scan(size, temperatures, coupling: float = 1.0, n_equilibrate: int = 1000, n_measure: int = 50,
                     measure_every: int = 10, periodic: bool = True, seed: int = 0, bias_mode: str = "physical",
                     initial: str = "up", algorithm: str = "gibbs", *, couplings=None, field=None, replicas: int = 1,
                     correlation: bool = False, improved: bool = False) -> dict:
    """GPU-resident form of :func:`demonstrate_phase_transition` (reference: ising.py:424-476) for lattices far
    beyond what a samples array can hold: one :class:`IsingModel2D` per temperature stays on the device, and
    |M|, E/N, chi = (<M^2> - <M>^2) N / T and C = (<E^2> - <E>^2) / (T^2 N) come from the device reductions
    (``tsu_ising2d_observables``) -- no spin ever crosses PCIe.  Returns arrays indexed like ``temperatures``.
    ``algorithm="swendsen_wang"``: ``n_equilibrate`` and ``measure_every`` count Swendsen-Wang steps (physical mode only).
    ``couplings`` / ``field``: the same quenched disorder (K7) at every temperature.  ``replicas=2``: a second model per
    temperature (seed ``seed + len(temperatures) + i``) runs beside the first, and the result gains the spin-glass
    observables ``overlap`` = <|q|>, ``overlap_sq`` = <q^2> and ``binder`` = (3 - <q^4> / <q^2>^2) / 2 of q = overlap / N;
    the other keys are those of the first replica, as with ``replicas=1``.
    ``correlation=True`` (a periodic lattice): the result gains ``chi_k`` = <|F_d|^2> / N and ``xi`` (both ``(n_T, 2)``, per axis) and
    ``xi_over_L`` = the mean of xi_d / L_d, from the k_min modes F_d of the spins (``replicas=1``) or of the overlap field
    (``replicas=2``) taken with every measurement (:meth:`IsingModel2D.fourier_modes`).
    ``improved=True`` (``algorithm="swendsen_wang"``): the measurement phase records the cluster sizes of its steps on the device
    and the result gains the improved estimators of :func:`_improved_summary`, averaged over the rows of EVERY step of the
    measurement phase, not only every ``measure_every``-th; all other keys keep their values bit for bit.
    """
    _check_algorithm(algorithm)
    _check_improved(improved, algorithm)
    if algorithm == "swendsen_wang_ghost":
        _refuse_ghost_2d()
    if replicas not in (1, 2):
        raise ValueError("replicas must be 1 or 2")
    if correlation:
        _check_correlation((bool(periodic),))
    disordered = couplings is not None or field is not None
    if algorithm == "swendsen_wang":
        if disordered:
            raise _hip.UnsupportedError("Swendsen-Wang cluster updates do not take a disordered lattice (couplings / field)")
        _check_cluster_model(0.0, bias_mode)
    temperatures = np.asarray(temperatures, dtype=float)
    rows, cols = (size, size) if np.isscalar(size) else tuple(size)
    disorder = None
    if disordered:  # validated once, before any device call
        disorder = _disorder_arrays(rows, cols, bool(periodic), float(coupling), 0.0, bias_mode, couplings, field)
    out = {k: np.zeros(len(temperatures)) for k in ("magnetization", "energy", "susceptibility", "specific_heat")}
    out["temperatures"] = temperatures
    # all temperatures advance together: lattices small enough for the one-workgroup kernel share ONE launch per
    # batch of sweeps (one workgroup per temperature) and one synchronisation per measurement; the streams (seed + i,
    # own sweep counter) and hence the results are those of sweeping the models one after the other
    nT = len(temperatures)
    kw = {} if disorder is None else {"couplings": (disorder[0], disorder[1]), "field": disorder[2]}
    models = [IsingModel2D(size, coupling=coupling if disorder is None else 1.0, temperature=float(T), periodic=periodic,
                           seed=seed + k * nT + i, bias_mode=bias_mode, initial=initial, **kw)
              for k in range(replicas) for i, T in enumerate(temperatures)]

    def advance(n_sweeps):
        if algorithm == "swendsen_wang":
            _hip.cluster_sweep_batch([m._lat for m in models], n_sweeps, [m.coupling for m in models],
                                     [m.temperature for m in models], [m.seed for m in models], [m.cluster_count for m in models])
            for m in models:
                m.cluster_count += int(n_sweeps)
            return
        if disorder is not None:
            for m in models:
                m.gibbs_update(int(n_sweeps))
            return
        for m in models:
            m._lat.set_model(m.coupling, m.external_field, m.temperature, m._mode)
        _hip.sweep_batch([m._lat for m in models], n_sweeps, [m.seed for m in models], [m.sweep_count for m in models])
        for m in models:
            m.sweep_count += int(n_sweeps)

    if models:
        advance(int(n_equilibrate))
    Ms, Es = np.zeros((nT, n_measure)), np.zeros((nT, n_measure))
    Qs = np.zeros((nT, n_measure))
    F2s = np.zeros((nT, n_measure, 2))
    recs = [[] for _ in range(nT)]
    for m in models if improved else ():  # every lattice of the batch, so that it keeps its one-launch route
        _set_cluster_measure(m, True)
    for j in range(n_measure if models else 0):
        advance(int(measure_every))
        for i in range(nT if improved else 0):
            recs[i].append(models[i].cluster_record())
        for i, (sum_s, sum_bonds) in enumerate(_hip.observables_batch([m._lat for m in models[:nT]])):
            Ms[i, j] = sum_s / models[i].n_spins
            if disorder is not None:
                Es[i, j] = models[i].energy()
            else:
                Es[i, j] = -models[i].coupling * float(sum_bonds) - models[i].external_field * float(sum_s)
            if replicas == 2:
                Qs[i, j] = models[i].overlap(models[nT + i])
            if correlation:
                F2s[i, j] = np.abs(models[i].fourier_modes(models[nT + i] if replicas == 2 else None)) ** 2
    del models
    out = _scan_summary(out, rows * cols, Ms, Es, Qs if replicas == 2 else None)
    if improved:
        _improved_summary(out, rows * cols, recs, ghost=False)
    if correlation:
        N = rows * cols
        f2 = np.mean((Qs if replicas == 2 else Ms) ** 2, axis=1) * float(N) ** 2
        _correlation_summary(out, N, (rows, cols), (bool(periodic),) * 2, f2, np.mean(F2s, axis=1))
    return out


def _scan_summary(out: dict, N: int, Ms, Es, Qs=None) -> dict:
    """Fill temperature_scan's keys from the per-temperature series Ms (M / N), Es (E) and, for two replicas, Qs (q / N)."""
    for i, T in enumerate(out["temperatures"]):
        out["magnetization"][i] = np.mean(np.abs(Ms[i]))
        out["energy"][i] = np.mean(Es[i]) / N
        out["susceptibility"][i] = (np.mean(Ms[i] ** 2) - np.mean(np.abs(Ms[i])) ** 2) * N / T
        out["specific_heat"][i] = (np.mean(Es[i] ** 2) - np.mean(Es[i]) ** 2) / (T ** 2 * N)
    if Qs is not None:
        q2 = np.mean(Qs ** 2, axis=1)
        out["overlap"] = np.mean(np.abs(Qs), axis=1)
        out["overlap_sq"] = q2
        with np.errstate(divide="ignore", invalid="ignore"):
            out["binder"] = 0.5 * (3.0 - np.mean(Qs ** 4, axis=1) / q2 ** 2)
    return out


def _improved_summary(out: dict, N: int, recs, ghost: bool) -> dict:
    """The scans' improved keys from recs[i], the cluster records of temperature i (one per measurement, each with the rows of
    ``measure_every`` steps; the means run over all rows): ``m2_improved`` = <m2>; ``chi_improved`` = N m2_improved / T at zero
    field, N (m2_improved - m_improved^2) / T with a ghost; ``binder_improved`` = (3 - <m4> / <m2>^2) / 2, zero field only;
    ``m_improved`` = <m>, ghost only (m2, m4, m: :func:`cluster_estimators`); ``mean_cluster_size`` = <sum |C|^2> / N;
    ``largest_cluster`` = <largest> / N, the fraction of the lattice in the largest free cluster; ``n_clusters`` = <n_clusters>."""
    nT = len(out["temperatures"])
    keys = ["m2_improved", "chi_improved", "mean_cluster_size", "largest_cluster", "n_clusters"] + (["m_improved"] if ghost else ["binder_improved"])
    for k in keys:
        out[k] = np.full(nT, np.nan)
    for i, T in enumerate(out["temperatures"]):
        if not recs[i]:
            continue
        rec = {k: np.concatenate([r[k] for r in recs[i]]) for k in _hip.CLUSTER_RECORD_FIELDS}
        rec["n_spins"] = N
        est = cluster_estimators(rec)
        m2 = float(np.mean(est["m2"]))
        out["m2_improved"][i] = m2
        if ghost:
            m = float(np.mean(est["m"]))
            out["m_improved"][i] = m
            out["chi_improved"][i] = N * (m2 - m * m) / T
        else:
            out["chi_improved"][i] = N * m2 / T
            out["binder_improved"][i] = 0.5 * (3.0 - float(np.mean(est["m4"])) / m2 ** 2)
        out["mean_cluster_size"][i] = float(np.mean(est["mean_cluster_size"]))
        out["largest_cluster"][i] = float(np.mean(rec["largest"])) / N
        out["n_clusters"][i] = float(np.mean(rec["n_clusters"]))
    return out


def _disorder_arrays_3d(shape, periodic, coupling: float, external_field: float, couplings, field):
    """Validate K8 disorder (before any device call) and round it once to fp32: (J_right, J_down, J_layer, h or None).
    ``periodic`` is the triple (p_z, p_r, p_c)."""
    if couplings is not None and coupling != 1.0:
        raise ValueError("give either couplings=(J_right, J_down, J_layer) or a scalar coupling, not both")
    if field is not None and external_field != 0.0:
        raise ValueError("give either field= or a non-zero external_field, not both")
    for p, n, name in zip(periodic, shape, ("depth", "rows", "cols")):
        if p and (n % 2 or n < 4):
            raise _hip.UnsupportedError(f"a periodic axis needs an even length >= 4 ({name} = {n})")

    def arr(a, name):
        a = np.asarray(a, dtype=np.float64)
        if a.shape != shape:
            raise ValueError(f"{name} must have shape {shape}, got {a.shape}")
        if not np.all(np.isfinite(a)):
            raise ValueError(f"{name} must be finite")
        with np.errstate(over="ignore"):
            a32 = a.astype(np.float32)
        if not np.all(np.isfinite(a32)):
            raise ValueError(f"{name} overflows float32")
        return a32

    if couplings is not None:
        if len(couplings) != 3:
            raise ValueError("couplings must be a triple (J_right, J_down, J_layer)")
        jr, jd, jl = arr(couplings[0], "J_right"), arr(couplings[1], "J_down"), arr(couplings[2], "J_layer")
    else:
        if not np.isfinite(np.float32(coupling)):
            raise ValueError("coupling must be finite in float32")
        jr, jd, jl = (np.full(shape, coupling, dtype=np.float32) for _ in range(3))
        if not periodic[2]:
            jr[:, :, -1] = 0.0
        if not periodic[1]:
            jd[:, -1, :] = 0.0
        if not periodic[0]:
            jl[-1, :, :] = 0.0
    if not periodic[2] and np.any(jr[:, :, -1] != 0):
        raise ValueError("open cols axis: the last column of J_right must be 0")
    if not periodic[1] and np.any(jd[:, -1, :] != 0):
        raise ValueError("open rows axis: the last row of J_down must be 0")
    if not periodic[0] and np.any(jl[-1, :, :] != 0):
        raise ValueError("open depth axis: the last layer of J_layer must be 0")
    if field is not None:
        h = arr(field, "field")
    else:
        if not np.isfinite(np.float32(external_field)):
            raise ValueError("external_field must be finite in float32")
        h = np.full(shape, external_field, dtype=np.float32) if external_field != 0.0 else None
    return jr, jd, jl, h


def _check_cluster_field_3d(h) -> None:
    """Swendsen-Wang samples the zero-field measure: refuse a stored field before the device is touched."""
    if h is not None and np.any(h != 0):
        raise _hip.UnsupportedError("Swendsen-Wang cluster updates need zero field (a field would need a ghost spin)")


def _shape_3d(size):
    shape = (size,) * 3 if np.isscalar(size) else tuple(int(n) for n in size)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"size must be an int or (depth, rows, cols) of positive ints, got {size!r}")
    return tuple(int(n) for n in shape)


class IsingModel3D:
    """A cubic lattice with quenched disorder that lives on the GPU between calls (K8; physical mode).

    ``IsingModel3D(size=(D, R, C), couplings=(J_right, J_down, J_layer), field=h, temperature=T)``: ``(D, R, C)`` arrays,
    ``J_right[z, r, c]`` couples (z, r, c) to (z, r, c+1), ``J_down`` to (z, r+1, c), ``J_layer`` to (z+1, r, c), ``field`` is the
    site's field.  ``periodic`` is a bool or a triple (p_z, p_r, p_c); a periodic axis wraps and needs an even length >= 4, on an
    open axis the last slice of that axis's J must be 0.  Uniform ``coupling=`` / ``external_field=`` are the constant-array case
    of the same kernel.  The arrays are rounded once to float32 (``disorder`` returns the rounded copies).
    ``gibbs_update()`` = one checkerboard heat-bath sweep; ``cluster_update()`` = one Swendsen-Wang step on the stored couplings
    (zero field only; its own counter ``cluster_count``); ``ghost_cluster_update()`` = one ghost-spin Swendsen-Wang step on the
    couplings and the field (the same counter); ``energy()`` / ``magnetization()`` / ``overlap(other)`` are device
    reductions; ``equilibrate(T)`` sets the temperature, runs ``n_sweeps`` sweeps (or SW steps, ``algorithm="swendsen_wang"`` /
    ``"swendsen_wang_ghost"``) and returns ``self``.
    """

    def __init__(self, size, coupling: float = 1.0, temperature: float = 1.0, periodic=True, external_field: float = 0.0,
                 seed: Optional[int] = None, initial: str = "random", *, couplings=None, field=None):
        if not temperature > 0:
            raise ValueError("Temperature must be positive")
        self.depth, self.rows, self.cols = self.shape = _shape_3d(size)
        self.n_spins = self.depth * self.rows * self.cols
        self.coupling = float(coupling)
        self.temperature = float(temperature)
        self.external_field = float(external_field)
        self.periodic = _hip.periodic_axes(periodic)
        if initial not in ("random", "up", "down"):
            raise ValueError("initial must be 'random', 'up' or 'down'")
        self._disorder = _disorder_arrays_3d(self.shape, self.periodic, self.coupling, self.external_field, couplings, field)
        self.seed = int(seed) if seed is not None else (
            int(np.random.randint(0, 2 ** 31 - 1)) | (int(np.random.randint(0, 2 ** 31 - 1)) << 31))
        self.sweep_count = 0
        self.cluster_count = 0
        self._measuring = False  # the handle's cluster-size record switch
        self._lat = _hip.Lattice3D(self.depth, self.rows, self.cols, self.periodic)
        if initial == "random":
            self._lat.randomize(self.seed)
        else:
            self._lat.fill(1 if initial == "up" else -1)
        self._lat.set_disorder(*self._disorder)

    @property
    def disorder(self):
        """(J_right, J_down, J_layer, h or None) as stored on the device (float32 copies)."""
        return tuple(None if a is None else a.copy() for a in self._disorder)

    def set_disorder(self, couplings=None, field=None) -> "IsingModel3D":
        """Replace the quenched disorder (``couplings=None``: uniform ``coupling``; ``field=None``: ``external_field``);
        the spins and counters are kept."""
        d = _disorder_arrays_3d(self.shape, self.periodic, self.coupling, self.external_field, couplings, field)
        self._lat.set_disorder(*d)
        self._disorder = d
        return self

    def gibbs_update(self, n_sweeps: int = 1) -> "IsingModel3D":
        self._lat.sweep(self.temperature, int(n_sweeps), self.seed, self.sweep_count)
        self.sweep_count += int(n_sweeps)
        return self

    def cluster_update(self, n_steps: int = 1, measure: bool = False) -> "IsingModel3D":
        """n_steps Swendsen-Wang steps on the stored couplings; the heat-bath stream and ``sweep_count`` are not touched.
        ``measure=True``: the same spins, and one cluster-size row per step for :meth:`cluster_record`."""
        _check_cluster_field_3d(self._disorder[3])
        _set_cluster_measure(self, measure)
        self._lat.cluster_sweep(self.temperature, int(n_steps), self.seed, self.cluster_count)
        self.cluster_count += int(n_steps)
        return self

    def ghost_cluster_update(self, n_steps: int = 1, measure: bool = False) -> "IsingModel3D":
        """n_steps ghost-spin Swendsen-Wang steps on the stored couplings and field: every site is also bonded to a ghost spin
        fixed at +1 with coupling h_i, and a cluster that reaches the ghost does not flip.  Samples exp(-E / T) / Z of
        :meth:`energy`; with zero field these are the steps of :meth:`cluster_update`.  Advances ``cluster_count``, the counter
        the two kinds of cluster step share.  ``measure=True``: the same spins, and one cluster-size row per step for
        :meth:`cluster_record` (the sites frozen to the ghost in ``n_frozen`` / ``m_frozen``)."""
        _set_cluster_measure(self, measure)
        self._lat.cluster_sweep_field(self.temperature, int(n_steps), self.seed, self.cluster_count)
        self.cluster_count += int(n_steps)
        return self

    def cluster_record(self) -> dict:
        """The cluster-size record of the last measured call (:meth:`IsingModel2D.cluster_record`); with ghost-spin steps
        ``n_frozen`` sites of total spin ``m_frozen`` hang on the ghost and the other words count the free clusters only."""
        rec = self._lat.cluster_record()
        rec["n_spins"] = self.n_spins
        return rec

    def equilibrate(self, temperature: Optional[float] = None, n_sweeps: int = 1000,
                    algorithm: str = "gibbs") -> "IsingModel3D":
        _check_algorithm(algorithm)
        if algorithm == "swendsen_wang":
            _check_cluster_field_3d(self._disorder[3])
        if temperature is not None:
            if not temperature > 0:
                raise ValueError("Temperature must be positive")
            self.temperature = float(temperature)
        if algorithm == "swendsen_wang":
            return self.cluster_update(n_sweeps)
        if algorithm == "swendsen_wang_ghost":
            return self.ghost_cluster_update(n_sweeps)
        return self.gibbs_update(n_sweeps)

    def magnetization(self) -> float:
        return self._lat.sum_spins() / self.n_spins

    def energy(self) -> float:
        return self._lat.energy()

    def overlap(self, other: "IsingModel3D") -> float:
        """q / N = sum_i s_i s'_i / N with another model of the same shape (a device reduction)."""
        if other.shape != self.shape:
            raise ValueError(f"overlap needs equal shapes, got {self.shape} and {other.shape}")
        return self._lat.overlap(other._lat) / self.n_spins

    def link_overlap(self, other: "IsingModel3D") -> float:
        """q_l = L / N_b with another model of the same shape and periodic axes (:meth:`IsingModel2D.link_overlap`)."""
        if other.shape != self.shape or tuple(other.periodic) != tuple(self.periodic):
            raise ValueError(f"link_overlap needs equal shapes and periodic axes, got {self.shape} and {other.shape}")
        L, nb = self._lat.link_overlap(other._lat)
        return L / nb

    def axis_profiles(self, other: Optional["IsingModel3D"] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(P_z, P_r, P_c): exact int64 sums of the spins (of s s' with ``other``) over the other two axes, on the device."""
        if other is not None and other.shape != self.shape:
            raise ValueError(f"axis_profiles needs equal shapes, got {self.shape} and {other.shape}")
        return self._lat.profiles(None if other is None else other._lat)

    def fourier_modes(self, other: Optional["IsingModel3D"] = None) -> np.ndarray:
        """complex128 (3,): the k_min = 2 pi / L_d modes of the three axis profiles (NaN on an open axis), summed on the host from
        the device's profiles in the fixed order of the ladders' mode pass."""
        return _kmin_modes(self.axis_profiles(other), self.periodic)

    @property
    def spins(self) -> np.ndarray:
        return self._lat.get_spins()

    @spins.setter
    def spins(self, value):
        v = np.asarray(value).reshape(self.shape)
        if not np.all((v == 1) | (v == -1)):
            raise ValueError("spins must be +1 / -1")
        self._lat.set_spins(v.astype(np.int8))


def temperature_scan_3d(size, temperatures, coupling: float = 1.0, n_equilibrate: int = 1000, n_measure: int = 50,
                        measure_every: int = 10, periodic=True, seed: int = 0, initial: str = "up", algorithm: str = "gibbs", *,
                        couplings=None, field=None, replicas: int = 1, correlation: bool = False,
                        external_field: float = 0.0, improved: bool = False) -> dict:
    """:func:`temperature_scan` for a cubic lattice (K8): one :class:`IsingModel3D` per temperature stays on the device and
    |M|, E/N, chi and C come from the device reductions.  ``couplings`` / ``field``: the same quenched disorder at every
    temperature.  Model i of replica k has seed ``seed + k len(temperatures) + i``.  ``replicas=2``: the result gains
    ``overlap`` = <|q|>, ``overlap_sq`` = <q^2> and ``binder`` = (3 - <q^4> / <q^2>^2) / 2 of q = overlap / N; the other keys are
    those of the first replica.  ``algorithm="swendsen_wang"``: ``n_equilibrate`` and ``measure_every`` count Swendsen-Wang steps
    on the couplings (zero field only); lattices of at most 16384 sites advance together, one launch per batch of steps.
    ``algorithm="swendsen_wang_ghost"``: the same with ghost-spin steps (:meth:`IsingModel3D.ghost_cluster_update`), which take
    ``field=`` / ``external_field=``.
    ``correlation=True`` (at least one periodic axis): the result gains ``chi_k`` = <|F_d|^2> / N and ``xi`` (both ``(n_T, 3)``, NaN on
    an open axis) and ``xi_over_L`` = the mean of xi_d / L_d over the periodic axes, from the k_min modes of the spins
    (``replicas=1``) or of the overlap field (``replicas=2``) taken with every measurement.
    ``improved=True`` (``algorithm="swendsen_wang"`` or ``"swendsen_wang_ghost"``): the measurement phase records the cluster
    sizes of its steps on the device and the result gains the improved estimators of :func:`_improved_summary`, averaged over the
    rows of EVERY step of the measurement phase, not only every ``measure_every``-th; all other keys keep their values bit for
    bit."""
    _check_algorithm(algorithm)
    _check_improved(improved, algorithm)
    if replicas not in (1, 2):
        raise ValueError("replicas must be 1 or 2")
    temperatures = np.asarray(temperatures, dtype=float)
    if np.any(~(temperatures > 0)):
        raise ValueError("Temperature must be positive")
    shape = _shape_3d(size)
    if correlation:
        _check_correlation(_hip.periodic_axes(periodic))
    # validated once, before any device call
    disorder = _disorder_arrays_3d(shape, _hip.periodic_axes(periodic), float(coupling), float(external_field), couplings, field)
    if algorithm == "swendsen_wang":
        _check_cluster_field_3d(disorder[3])
    out = {k: np.zeros(len(temperatures)) for k in ("magnetization", "energy", "susceptibility", "specific_heat")}
    out["temperatures"] = temperatures
    nT = len(temperatures)
    models = [IsingModel3D(shape, temperature=float(T), periodic=periodic, seed=seed + k * nT + i, initial=initial,
                           couplings=disorder[:3], field=disorder[3])
              for k in range(replicas) for i, T in enumerate(temperatures)]

    def advance(n):
        if algorithm != "gibbs":  # the streams (seed, own step counter) are those of stepping the models one by one
            batch = _hip.cluster_sweep_batch_3d if algorithm == "swendsen_wang" else _hip.cluster_sweep_field_batch_3d
            batch([m._lat for m in models], n, [m.temperature for m in models], [m.seed for m in models],
                  [m.cluster_count for m in models])
            for m in models:
                m.cluster_count += int(n)
            return
        for m in models:
            m.gibbs_update(int(n))

    if models:
        advance(int(n_equilibrate))
    Ms, Es, Qs = np.zeros((nT, n_measure)), np.zeros((nT, n_measure)), np.zeros((nT, n_measure))
    F2s = np.zeros((nT, n_measure, 3))
    recs = [[] for _ in range(nT)]
    for m in models if improved else ():  # every lattice of the batch, so that it keeps its one-launch route
        _set_cluster_measure(m, True)
    for j in range(n_measure if models else 0):
        advance(int(measure_every))
        for i in range(nT if improved else 0):
            recs[i].append(models[i].cluster_record())
        for i in range(nT):
            Ms[i, j] = models[i].magnetization()
            Es[i, j] = models[i].energy()
            if replicas == 2:
                Qs[i, j] = models[i].overlap(models[nT + i])
            if correlation:
                F2s[i, j] = np.abs(models[i].fourier_modes(models[nT + i] if replicas == 2 else None)) ** 2
    del models
    N = shape[0] * shape[1] * shape[2]
    out = _scan_summary(out, N, Ms, Es, Qs if replicas == 2 else None)
    if improved:
        _improved_summary(out, N, recs, ghost=algorithm == "swendsen_wang_ghost")
    if correlation:
        f2 = np.mean((Qs if replicas == 2 else Ms) ** 2, axis=1) * float(N) ** 2
        _correlation_summary(out, N, shape, _hip.periodic_axes(periodic), f2, np.mean(F2s, axis=1))
    return out


_PT_INITIAL = {"random": 0, "up": 1, "down": -1}


def _cluster_move_args(cluster_moves, cluster_max_temperature, ladders: int):
    """(every, t_max) of the replica cluster moves, validated on the host."""
    if isinstance(cluster_moves, bool) or not isinstance(cluster_moves, (int, np.integer)) or cluster_moves < 0:
        raise ValueError("cluster_moves must be an integer >= 0 (0: off; n: a pass after the sweeps of every n-th round)")
    t_max = float("inf")
    if cluster_max_temperature is not None:
        try:
            t_max = float(cluster_max_temperature)
        except (TypeError, ValueError):
            raise ValueError("cluster_max_temperature must be a positive number") from None
        if not t_max > 0:
            raise ValueError("cluster_max_temperature must be a positive number")
    if cluster_moves >= 1 and ladders != 2:
        raise ValueError("cluster moves exchange clusters between the two replicas at one temperature: they need ladders=2")
    return int(cluster_moves), t_max


class _LatticeTempering:
    """What :class:`LatticeTempering` and :class:`LatticeTempering3D` share: everything but the shape, the disorder and the 2-D
    cluster moves.  A subclass parses its shape, calls ``_check_ladder``, validates its disorder into ``self._disorder`` and hands
    its new handle to ``_start``."""

    def _check_ladder(self, temperatures, ladders, initial):
        T = np.asarray(temperatures, dtype=float).ravel()
        if not 2 <= T.size <= 256:
            raise ValueError(f"parallel tempering needs 2 to 256 temperatures, got {T.size}")
        if not np.all(np.isfinite(T) & (T > 0)):
            raise ValueError("Temperature must be positive")
        if ladders not in (1, 2):
            raise ValueError("ladders must be 1 or 2")
        if initial not in _PT_INITIAL:
            raise ValueError("initial must be 'random', 'up' or 'down'")
        self.temperatures = T
        self.ladders = int(ladders)

    def _start(self, pt, seed, initial):
        self._pt = pt
        self.seed = int(seed) if seed is not None else (
            int(np.random.randint(0, 2 ** 31 - 1)) | (int(np.random.randint(0, 2 ** 31 - 1)) << 31))
        pt.set_disorder(*self._disorder)
        pt.set_temperatures(self.temperatures)
        if getattr(self, "cluster_moves", 0):  # 2-D only
            pt.set_cluster_moves(self.cluster_moves, self.cluster_max_temperature)
        if self.link_overlap:
            pt.set_link_overlap(True)
        if self.correlation:  # the tables are made here, on the host
            pt.set_correlation(True, [_kmin_tables(n) if per else None for n, per in zip(pt.shape, self._axes_periodic())])
        pt.init(self.seed, _PT_INITIAL[initial])

    def _axes_periodic(self):
        p = self.periodic
        return tuple(p) if isinstance(p, tuple) else (bool(p),) * 2

    link_overlap = False  # history() also has q_link

    def _set_link_overlap(self, link_overlap):
        """Before any device call: keep the flag, refuse a single ladder."""
        self.link_overlap = bool(link_overlap)
        if self.link_overlap and self.ladders != 2:
            raise ValueError("link_overlap=True compares the two replicas at one temperature: it needs ladders=2")

    def _set_correlation(self, correlation):
        """Before any device call: keep the flag, refuse a lattice without a periodic axis."""
        self.correlation = bool(correlation)
        if self.correlation:
            _check_correlation(self._axes_periodic())

    def run(self, n_rounds: int, swap_interval: int = 10, swap: bool = True, record: bool = True):
        """n_rounds rounds of swap_interval sweeps each; with ``record`` returns ``history()`` (ladder 0), else None."""
        self._pt.run(int(n_rounds), int(swap_interval), swap, record)
        return self.history() if record else None

    def history(self, ladder: int = 0) -> dict:
        """The rounds recorded by the last ``run`` as (n_rounds, R) arrays, per slot: ``E`` (float64 energy), ``M`` (int64 sum of
        spins), ``walker`` (which walker of the ladder sat there) and, with two ladders, ``q`` (int64 overlap of the two ladders'
        walkers at that slot).  With ``correlation=True`` also ``modes``: complex128 (n_rounds, R, n_axes), the k_min mode of each
        axis profile of the walker at that slot (one ladder: of its spins; two: of the overlap field; NaN on an open axis).  With
        ``link_overlap=True`` also ``q_link``: int64 (n_rounds, R), L of the two walkers at that slot (q_l = L / N_b)."""
        h = self._pt.history()
        out = {k: np.ascontiguousarray(h[k][:, ladder]) for k in ("E", "M", "walker")}
        if h["q"] is not None:
            out["q"] = h["q"]
        if "q_link" in h:
            out["q_link"] = h["q_link"]
        if self.correlation:
            per = np.asarray(self._axes_periodic(), dtype=bool)
            got = self._pt.history_modes()
            modes = np.full(got.shape[:2] + (per.size,), complex(np.nan, np.nan), dtype=np.complex128)
            modes[:, :, per] = got
            out["modes"] = modes
        return out

    def axis_profiles(self, slot: int) -> tuple:
        """int64 axis profiles of the walker now at ``slot`` (two ladders: of the product of the two walkers there)."""
        self._check_slot(slot, 0)
        return self._pt.profiles(slot)

    @property
    def acceptance(self) -> np.ndarray:
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

    def _check_slot(self, slot, ladder):
        if not (0 <= slot < self.temperatures.size and 0 <= ladder < self.ladders):
            raise ValueError(f"slot {slot} / ladder {ladder} out of range ({self.ladders} ladder(s) of {self.temperatures.size})")

    def spins(self, slot: int, ladder: int = 0) -> np.ndarray:
        """Spins of the walker now at ``slot``, in the lattice's shape."""
        self._check_slot(slot, ladder)
        return self._pt.get_spins(ladder, slot)

    def energy(self, slot: int, ladder: int = 0) -> float:
        """Energy of the walker now at ``slot`` (the device's fixed-order float64 sum)."""
        self._check_slot(slot, ladder)
        E, _ = self._pt.energies()
        return float(E[ladder, self._pt.stats()["walker_at_slot"][ladder, slot]])


def _tempering_scan(pt, temperatures, n_equilibrate, n_measure, measure_every, swap) -> dict:
    """The body of the tempering scans on a fresh ladder ``pt``, closed at the end: the equilibration rounds, the recorded rounds
    and temperature_scan's summary of them, plus ``cluster_flipped`` where the ladder makes cluster moves (2-D only)."""
    try:
        pt.run(int(n_equilibrate) // int(measure_every), int(measure_every), swap=swap, record=False)
        pt.run(int(n_measure), int(measure_every), swap=swap, record=True)
        hist = pt._pt.history()
        N = pt.n_spins
        out = {k: np.zeros(len(temperatures)) for k in ("magnetization", "energy", "susceptibility", "specific_heat")}
        out["temperatures"] = temperatures
        Ms = np.ascontiguousarray(hist["M"][:, 0].T) / N
        Es = np.ascontiguousarray(hist["E"][:, 0].T)
        Qs = np.ascontiguousarray(hist["q"].T) / N if pt.ladders == 2 else None
        out = _scan_summary(out, N, Ms, Es, Qs)
        if pt.link_overlap:
            out["link_overlap"] = np.mean(hist["q_link"], axis=0) / lattice_bond_count(pt._pt.shape, pt._axes_periodic())
        if pt.correlation:
            F2 = np.mean(np.abs(pt.history()["modes"]) ** 2, axis=0)
            f2 = np.mean((Qs if pt.ladders == 2 else Ms) ** 2, axis=1) * float(N) ** 2
            _correlation_summary(out, N, pt._pt.shape, pt._axes_periodic(), f2, F2)
        out["swap_acceptance"] = pt.acceptance
        out["round_trips"] = pt.round_trips
        if getattr(pt, "cluster_moves", 0):
            st = pt.cluster_stats
            with np.errstate(divide="ignore", invalid="ignore"):
                out["cluster_flipped"] = st["flipped"] / (st["passes"] * float(N))
    finally:
        pt._pt.close()
    return out


class LatticeTempering(_LatticeTempering):
    """Parallel tempering (replica exchange) of a disordered lattice on the GPU (K7, physical mode).

    ``ladders`` (1 or 2) ladders of ``R = len(temperatures)`` walkers (2 ... 256) share one quenched disorder: ``couplings=(J_right,
    J_down)`` and ``field`` as for :class:`IsingModel2D`, or the uniform ``coupling`` / ``external_field``, validated and rounded to
    float32 before any device call.  Walker w of ladder k is model ``k R + w`` of ``temperature_scan(seed=seed)`` (same Philox key,
    initial draw and sweep counter) and starts at slot w.  ``run(n_rounds, swap_interval)``: each round sweeps every walker
    ``swap_interval`` times at the temperature of its slot, computes every energy and makes one pass of swap attempts over the
    adjacent slots of each ladder in the reference's order and rule (``GibbsSampler.parallel_tempering``, gibbs.py:309-323), all on
    the device without a host synchronisation.  A swap exchanges the walkers' temperatures, never their spins.

    ``cluster_moves=n >= 1`` (needs ``ladders=2``) adds Houdayer's isoenergetic cluster move (Eur. Phys. J. B 22, 479 (2001)): every
    n-th round, after the sweeps and before the energies, the two replicas at each temperature ``<= cluster_max_temperature``
    (default: all) exchange randomly chosen connected clusters of the sites where they differ (``q_x = a_x b_x = -1``), each
    cluster with probability 1/2.  The sum of the two energies and every ``q_x`` are unchanged, so the move needs no accept / reject
    step; it is a rearrangement between the replicas that the single-spin sweeps would take very long to find.  It is useful only
    while the ``q = -1`` sites do not percolate (site threshold of the square lattice, 0.593): above that one cluster spans the
    lattice and the move is close to exchanging the two replicas, which changes nothing.  That is physics, not a fault; it is why
    the cut-off exists, and ``cluster_stats`` shows it: ``flipped / (passes * N)`` near 1/2 at a slot says it percolates there.
    """

    def __init__(self, size, temperatures, *, couplings=None, field=None, coupling: float = 1.0, external_field: float = 0.0,
                 periodic: bool = True, seed: Optional[int] = None, initial: str = "random", ladders: int = 1,
                 cluster_moves: int = 0, cluster_max_temperature: Optional[float] = None, correlation: bool = False,
                 link_overlap: bool = False):
        self.rows, self.cols = (size, size) if np.isscalar(size) else tuple(size)
        self.n_spins = self.rows * self.cols
        self._check_ladder(temperatures, ladders, initial)
        self.cluster_moves, self.cluster_max_temperature = _cluster_move_args(cluster_moves, cluster_max_temperature, ladders)
        self.periodic = bool(periodic)
        self._set_correlation(correlation)
        self._set_link_overlap(link_overlap)
        self._disorder = _disorder_arrays(self.rows, self.cols, self.periodic, float(coupling), float(external_field), "physical",
                                          couplings, field)
        self._start(_hip.TemperingLattice(self.rows, self.cols, self.periodic, self.temperatures.size, self.ladders), seed, initial)

    def cluster_move(self) -> None:
        """One replica cluster pass now over the participating slots (needs ``cluster_moves >= 1``)."""
        self._pt.cluster_move()

    @property
    def cluster_stats(self) -> dict:
        """Per slot since the start: ``passes`` taken, ``clusters`` found and sites ``flipped`` (per replica) by the cluster moves."""
        st = self._pt.cluster_stats()
        return {k: st[k] for k in ("passes", "clusters", "flipped")}


def tempering_scan(size, temperatures, coupling: float = 1.0, n_equilibrate: int = 1000, n_measure: int = 50,
                   measure_every: int = 10, periodic: bool = True, seed: int = 0, bias_mode: str = "physical",
                   initial: str = "up", *, couplings=None, field=None, replicas: int = 1, swap: bool = True,
                   cluster_moves: int = 0, cluster_max_temperature: Optional[float] = None, correlation: bool = False,
                   link_overlap: bool = False) -> dict:
    """:func:`temperature_scan` of a disordered lattice with replica exchange between the temperatures (:class:`LatticeTempering`).

    One round = ``measure_every`` sweeps of every walker + one swap pass; ``n_equilibrate`` (a multiple of ``measure_every``)
    sweeps of rounds, then ``n_measure`` recorded rounds.  Returns temperature_scan's keys, computed with the same expressions from
    the walker at each temperature (``overlap``, ``overlap_sq``, ``binder`` for ``replicas=2``), plus ``swap_acceptance`` (per
    adjacent pair, ladders pooled) and ``round_trips`` (all walkers).  ``swap=False`` reproduces ``temperature_scan`` with the same
    arguments exactly.  ``cluster_moves`` / ``cluster_max_temperature`` as for :class:`LatticeTempering` (``replicas=2``); they add
    ``cluster_flipped``: the mean fraction of the sites a pass flipped per temperature, NaN where the slot does not take part.
    ``correlation=True``: ``chi_k``, ``xi`` and ``xi_over_L`` as for :func:`temperature_scan`, from the modes the ladder records on the
    device in every recorded round.  ``link_overlap=True`` (``replicas=2``) adds ``link_overlap``: the mean of q_l = L / N_b per
    temperature.
    """
    if replicas not in (1, 2):
        raise ValueError("replicas must be 1 or 2")
    if link_overlap and replicas != 2:
        raise ValueError("link_overlap=True compares the two replicas at one temperature: it needs replicas=2")
    if correlation:
        _check_correlation((bool(periodic),))
    _cluster_move_args(cluster_moves, cluster_max_temperature, replicas)
    if int(measure_every) < 1 or int(n_equilibrate) % int(measure_every):
        raise ValueError("n_equilibrate must be a multiple of measure_every")
    rows, cols = (size, size) if np.isscalar(size) else tuple(size)
    jr, jd, h = _disorder_arrays(rows, cols, bool(periodic), float(coupling), 0.0, bias_mode, couplings, field)
    temperatures = np.asarray(temperatures, dtype=float)
    pt = LatticeTempering((rows, cols), temperatures, couplings=(jr, jd), field=h, periodic=periodic, seed=seed, initial=initial,
                          ladders=replicas, cluster_moves=cluster_moves, cluster_max_temperature=cluster_max_temperature,
                          correlation=correlation, link_overlap=link_overlap)
    return _tempering_scan(pt, temperatures, n_equilibrate, n_measure, measure_every, swap)


class _PeriodicAxisError(_hip.UnsupportedError, ValueError):
    """The periodic-axis rule of K8 refused by the 3-D ladders on the host: the UnsupportedError every K8 entry point raises for
    it, and a ValueError like the rest of the ladders' argument validation."""


def _tempering_disorder_3d(shape, periodic, coupling, external_field, couplings, field):
    try:
        return _disorder_arrays_3d(shape, periodic, coupling, external_field, couplings, field)
    except _hip.UnsupportedError as e:
        raise _PeriodicAxisError(str(e)) from None


class LatticeTempering3D(_LatticeTempering):
    """Parallel tempering (replica exchange) of a disordered cubic lattice on the GPU (K8, physical mode): :class:`LatticeTempering`
    for the lattices of :class:`IsingModel3D`.

    ``ladders`` (1 or 2) ladders of ``R = len(temperatures)`` walkers (2 ... 256) share one quenched disorder:
    ``couplings=(J_right, J_down, J_layer)`` and ``field`` as for :class:`IsingModel3D`, or the uniform ``coupling`` /
    ``external_field``; ``periodic`` is a bool or a triple (p_z, p_r, p_c).  Everything is validated and rounded to float32 before
    any device call.  Walker w of ladder k is model ``k R + w`` of ``temperature_scan_3d(seed=seed)`` (same Philox key, initial
    draw and sweep counter) and starts at slot w.  ``run(n_rounds, swap_interval)``: each round sweeps every walker
    ``swap_interval`` times at the temperature of its slot (one launch per half-sweep for all walkers), computes every energy and
    makes one pass of swap attempts over the adjacent slots of each ladder by the rule of :class:`LatticeTempering`, all on the
    device without a host synchronisation.  A swap exchanges the walkers' temperatures, never their spins.  There are no replica
    cluster moves in 3-D: the q = -1 sites of a cubic lattice percolate (site threshold 0.3116) at every temperature of interest.
    """

    def __init__(self, size, temperatures, *, couplings=None, field=None, coupling: float = 1.0, external_field: float = 0.0,
                 periodic=True, seed: Optional[int] = None, initial: str = "random", ladders: int = 1, correlation: bool = False,
                 link_overlap: bool = False):
        self.depth, self.rows, self.cols = self.shape = _shape_3d(size)
        self.n_spins = self.depth * self.rows * self.cols
        self._check_ladder(temperatures, ladders, initial)
        self.periodic = _hip.periodic_axes(periodic)
        self._set_correlation(correlation)
        self._set_link_overlap(link_overlap)
        self._disorder = _tempering_disorder_3d(self.shape, self.periodic, float(coupling), float(external_field), couplings, field)
        self._start(_hip.TemperingLattice3D(self.depth, self.rows, self.cols, self.periodic, self.temperatures.size, self.ladders),
                    seed, initial)


def tempering_scan_3d(size, temperatures, coupling: float = 1.0, n_equilibrate: int = 1000, n_measure: int = 50,
                      measure_every: int = 10, periodic=True, seed: int = 0, initial: str = "up", *, couplings=None, field=None,
                      replicas: int = 1, swap: bool = True, correlation: bool = False, link_overlap: bool = False) -> dict:
    """:func:`temperature_scan_3d` with replica exchange between the temperatures (:class:`LatticeTempering3D`).

    One round = ``measure_every`` sweeps of every walker + one swap pass; ``n_equilibrate`` (a multiple of ``measure_every``)
    sweeps of rounds, then ``n_measure`` recorded rounds.  Returns temperature_scan_3d's keys, computed with the same expressions
    from the walker at each temperature (``overlap``, ``overlap_sq``, ``binder`` for ``replicas=2``), plus ``swap_acceptance`` (per
    adjacent pair, ladders pooled) and ``round_trips`` (all walkers).  ``swap=False`` reproduces ``temperature_scan_3d`` with the
    same arguments exactly.  ``correlation=True``: ``chi_k``, ``xi`` and ``xi_over_L`` as for :func:`temperature_scan_3d`, from the
    modes the ladder records on the device in every recorded round.  ``link_overlap=True`` (``replicas=2``) adds ``link_overlap``: the
    mean of q_l = L / N_b per temperature.
    """
    if replicas not in (1, 2):
        raise ValueError("replicas must be 1 or 2")
    if link_overlap and replicas != 2:
        raise ValueError("link_overlap=True compares the two replicas at one temperature: it needs replicas=2")
    if int(measure_every) < 1 or int(n_equilibrate) % int(measure_every):
        raise ValueError("n_equilibrate must be a multiple of measure_every")
    shape = _shape_3d(size)
    if correlation:
        _check_correlation(_hip.periodic_axes(periodic))
    jr, jd, jl, h = _tempering_disorder_3d(shape, _hip.periodic_axes(periodic), float(coupling), 0.0, couplings, field)
    temperatures = np.asarray(temperatures, dtype=float)
    pt = LatticeTempering3D(shape, temperatures, couplings=(jr, jd, jl), field=h, periodic=periodic, seed=seed, initial=initial,
                            ladders=replicas, correlation=correlation, link_overlap=link_overlap)
    return _tempering_scan(pt, temperatures, n_equilibrate, n_measure, measure_every, swap)


# ---------------------------------------------------------------------------------------------------- tempering ensembles
ENSEMBLE_MAX_WALKERS = 65535  # samples x ladders x temperatures one launch covers


def edwards_anderson_samples(size, n_samples: int, kind: str = "bimodal", seed: int = 0, dims: int = 3, periodic=True):
    """Couplings of ``n_samples`` Edwards-Anderson disorder samples: a tuple ``(J_right, J_down)`` (``dims=2``) or ``(J_right, J_down,
    J_layer)`` (``dims=3``) of float32 arrays of shape ``(n_samples, *lattice)``, the ``couplings=`` of the ensembles.

    Sample s is drawn from ``np.random.default_rng([seed, s])`` in the order J_right, J_down, (J_layer), every bond of every site:
    ``kind="bimodal"`` gives +-1 with equal probability, ``"gaussian"`` a standard normal.  So sample s does not depend on
    ``n_samples``, and not on the boundary either: the bonds that would cross an open boundary (the last column of J_right, the last
    row of J_down, the last layer of J_layer) are drawn like the others, so the stream stays the same, and then stored as 0 where
    ``periodic`` (a bool, or one flag per axis in the lattice's axis order) says the axis is open, because the lattices refuse a
    non-zero bond there; on a periodic axis they are the wrap bonds."""
    if dims not in (2, 3):
        raise ValueError("dims must be 2 or 3")
    if kind not in ("bimodal", "gaussian"):
        raise ValueError("kind must be 'bimodal' or 'gaussian'")
    shape = (size,) * dims if np.isscalar(size) else tuple(int(n) for n in size)
    if len(shape) != dims or min(shape) < 1:
        raise ValueError(f"size must be an int or {dims} positive ints, got {size!r}")
    S = int(n_samples)
    if S < 1:
        raise ValueError("n_samples must be >= 1")
    per = (bool(periodic),) * dims if isinstance(periodic, (bool, np.bool_)) else tuple(bool(x) for x in periodic)
    if len(per) != dims:
        raise ValueError(f"periodic must be a bool or {dims} flags")
    out = [np.zeros((S,) + shape, np.float32) for _ in range(dims)]
    for smp in range(S):
        rng = np.random.default_rng([int(seed), smp])
        for a in out:
            a[smp] = (2.0 * rng.integers(0, 2, size=shape) - 1.0) if kind == "bimodal" else rng.standard_normal(shape)
    # out[j] holds the bonds along lattice axis dims - 1 - j (J_right: the last axis)
    for j, a in enumerate(out):
        axis = dims - 1 - j
        if not per[axis]:
            a[(slice(None),) * (axis + 1) + (-1,)] = 0.0
    return tuple(out)


def ensemble_seeds(seed: int, n_samples: int, ladders: int, n_temps: int) -> List[int]:
    """``seeds[s] = seed + s * ladders * n_temps``: the walkers of sample s take the keys seeds[s] .. seeds[s] + ladders * n_temps - 1,
    so no two walkers of the ensemble share a key."""
    return [int(seed) + s * int(ladders) * int(n_temps) for s in range(int(n_samples))]


def _sem(x) -> np.ndarray:
    """Standard error of the mean over the leading (sample) axis; NaN for a single sample."""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[0] < 2:
        return np.full(x.shape[1:], np.nan)
    return np.std(x, axis=0, ddof=1) / np.sqrt(x.shape[0])


def _jackknife(fn, *arrays):
    """(estimate, error) of ``fn(mean over samples of each array)``: the estimate from the full means, the error from the
    delete-one jackknife over the leading (sample) axis, sqrt((S - 1) / S * sum_i (theta_i - mean theta)^2); NaN for one sample."""
    arrays = [np.asarray(a, dtype=np.float64) for a in arrays]
    S = arrays[0].shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        est = np.asarray(fn(*[a.mean(axis=0) for a in arrays]), dtype=np.float64)
        if S < 2:
            return est, np.full(est.shape, np.nan)
        tot = [a.sum(axis=0) for a in arrays]
        th = np.stack([np.asarray(fn(*[(t - a[i]) / (S - 1) for t, a in zip(tot, arrays)]), dtype=np.float64) for i in range(S)])
        return est, np.sqrt((S - 1) / S * np.sum((th - th.mean(axis=0)) ** 2, axis=0))


def ensemble_summary(samples: dict, n_spins: Optional[int] = None, lengths=None, periodic=None) -> dict:
    """Disorder averages [.]_J over the leading sample axis of the per-sample arrays of a tempering-ensemble scan.

    Plain means, each with ``<key>_err`` = the standard error of the mean over samples, of whichever of these ``samples`` holds:
    ``energy`` [<e>], ``magnetization``, ``overlap`` [<|q|>], ``overlap_sq`` [<q^2>], ``link_overlap`` [q_l].  Ratios, averaged first
    and divided afterwards, each with a delete-one jackknife error over samples: ``binder`` = (3 - [<q^4>] / [<q^2>]^2) / 2 from
    ``overlap_4`` and ``overlap_sq``; and, from ``F2`` (<|F(k_min)|^2> per axis, NaN on open axes) and ``f2`` (<f_tot^2>) with
    ``n_spins``, ``lengths`` and ``periodic``: ``chi_k`` = [F2] / N (a plain mean, with its standard error), ``xi`` =
    :func:`correlation_length` of ([f2], [F2]) per axis and ``xi_over_L`` = its mean over the periodic axes of xi_d / L_d."""
    out = {}
    for k in ("energy", "magnetization", "overlap", "overlap_sq", "link_overlap"):
        if k in samples:
            x = np.asarray(samples[k], dtype=np.float64)
            out[k] = x.mean(axis=0)
            out[k + "_err"] = _sem(x)
    if "overlap_4" in samples and "overlap_sq" in samples:
        out["binder"], out["binder_err"] = _jackknife(lambda q4, q2: 0.5 * (3.0 - q4 / q2 ** 2), samples["overlap_4"], samples["overlap_sq"])
    if "F2" in samples and "f2" in samples:
        if n_spins is None or lengths is None or periodic is None:
            raise ValueError("the correlation averages need n_spins, lengths and periodic")
        per = np.asarray(periodic, dtype=bool)
        L = np.asarray(lengths, dtype=np.float64)
        F2 = np.asarray(samples["F2"], dtype=np.float64)
        out["chi_k"] = F2.mean(axis=0) / n_spins
        out["chi_k_err"] = _sem(F2) / n_spins
        out["xi"], out["xi_err"] = _jackknife(lambda f, F: correlation_length(f, F, L), samples["f2"], F2)
        out["xi_over_L"], out["xi_over_L_err"] = _jackknife(
            lambda f, F: np.mean(correlation_length(f, F, L)[..., per] / L[per], axis=-1), samples["f2"], F2)
    return out


class _LatticeTemperingEnsemble(_LatticeTempering):
    """What :class:`LatticeTemperingEnsemble` and :class:`LatticeTemperingEnsemble3D` share.  A subclass parses its shape into
    ``self.shape``, sets ``self.periodic`` and names the per-sample validation of its disorder (``_sample_disorder``) and its handle
    (``_handle``)."""

    def __init__(self, size, temperatures, *, couplings, field=None, periodic=True, seeds=None, seed: Optional[int] = None,
                 initial: str = "random", ladders: int = 1, correlation: bool = False, link_overlap: bool = False):
        self._parse_shape(size, periodic)
        self.n_spins = int(np.prod(self.shape))
        self._check_ladder(temperatures, ladders, initial)
        self._set_correlation(correlation)
        self._set_link_overlap(link_overlap)
        self._disorder = self._ensemble_disorder(couplings, field)
        S, R = self.n_samples, self.temperatures.size
        if S * self.ladders * R > ENSEMBLE_MAX_WALKERS:
            raise ValueError(f"{S} samples x {self.ladders} ladder(s) x {R} temperatures = {S * self.ladders * R} walkers: one ensemble "
                             f"holds at most {ENSEMBLE_MAX_WALKERS}")
        if seeds is not None and seed is not None:
            raise ValueError("give either seeds= (one per sample) or seed=, not both")
        if seeds is None:
            if seed is None:
                seed = int(np.random.randint(0, 2 ** 31 - 1)) | (int(np.random.randint(0, 2 ** 31 - 1)) << 31)
            seeds = ensemble_seeds(seed, S, self.ladders, R)
        seeds = [int(x) for x in seeds]
        if len(seeds) != S:
            raise ValueError(f"need one seed per sample ({S}), got {len(seeds)}")
        if any(not 0 <= x < 2 ** 64 for x in seeds):
            raise ValueError("seeds must fit an unsigned 64-bit integer")
        self.seeds = seeds
        pt = self._pt = self._handle()
        pt.set_disorder(*self._disorder)
        pt.set_temperatures(self.temperatures)
        if self.link_overlap:
            pt.set_link_overlap(True)
        if self.correlation:
            pt.set_correlation(True, [_kmin_tables(n) if per else None for n, per in zip(pt.shape, self._axes_periodic())])
        pt.init(self.seeds, _PT_INITIAL[initial])

    def _ensemble_disorder(self, couplings, field):
        """Before any device call: the sample count from the leading axis, then every sample through the ladders' validation."""
        nj = len(self.shape)
        if couplings is None or len(couplings) != nj:
            raise ValueError(f"couplings must be {nj} arrays of shape (n_samples,) + {self.shape}")
        arrs = [np.asarray(a) for a in couplings] + ([] if field is None else [np.asarray(field)])
        names = ["J_right", "J_down", "J_layer"][:nj] + ["field"]
        for a, name in zip(arrs, names):
            if a.ndim != nj + 1 or a.shape[1:] != self.shape:
                raise ValueError(f"{name} must have shape (n_samples,) + {self.shape}, got {a.shape}")
        S = arrs[0].shape[0]
        if S < 1:
            raise ValueError("an ensemble needs at least one disorder sample")
        for a, name in zip(arrs, names):
            if a.shape[0] != S:
                raise ValueError(f"{name} has {a.shape[0]} samples, J_right has {S}")
        self.n_samples = int(S)
        per = [self._sample_disorder(tuple(a[s] for a in arrs[:nj]), None if field is None else arrs[nj][s]) for s in range(S)]
        out = [np.stack([p[j] for p in per]) for j in range(nj)]
        return tuple(out) + (None if field is None else np.stack([p[nj] for p in per]),)

    def close(self) -> None:
        self._pt.close()

    def _check_sample(self, sample):
        if not 0 <= sample < self.n_samples:
            raise ValueError(f"sample {sample} out of range ({self.n_samples} samples)")

    def history(self, sample: Optional[int] = None, ladder: int = 0) -> dict:
        """The rounds recorded by the last ``run``, the keys of :meth:`LatticeTempering.history`: for one ``sample`` its ladder's
        arrays, (n_rounds, R) (``modes``: (n_rounds, R, n_axes)); for ``sample=None`` all samples, with a leading sample axis."""
        if sample is not None:
            self._check_sample(sample)
        h = self._pt.history()
        out = {k: np.ascontiguousarray(np.moveaxis(h[k][:, :, ladder], 1, 0)) for k in ("E", "M", "walker")}
        for k in ("q", "q_link"):
            if h.get(k) is not None:
                out[k] = np.ascontiguousarray(np.moveaxis(h[k], 1, 0))
        if self.correlation:
            per = np.asarray(self._axes_periodic(), dtype=bool)
            got = np.moveaxis(self._pt.history_modes(), 1, 0)
            modes = np.full(got.shape[:3] + (per.size,), complex(np.nan, np.nan), dtype=np.complex128)
            modes[..., per] = got
            out["modes"] = modes
        return out if sample is None else {k: np.ascontiguousarray(v[sample]) for k, v in out.items()}

    def axis_profiles(self, sample: int, slot: int) -> tuple:
        self._check_sample(sample)
        self._check_slot(slot, 0)
        return self._pt.profiles(sample, slot)

    @property
    def acceptance(self) -> np.ndarray:
        """(n_samples, R - 1): accepted / attempted swaps per adjacent pair of slots of each sample, its ladders pooled."""
        st = self._pt.stats()
        with np.errstate(divide="ignore", invalid="ignore"):
            return st["accepts"].sum(axis=1) / st["attempts"].sum(axis=1)

    @property
    def acceptance_pooled(self) -> np.ndarray:
        """(R - 1,): the same with all samples pooled."""
        st = self._pt.stats()
        with np.errstate(divide="ignore", invalid="ignore"):
            return st["accepts"].sum(axis=(0, 1)) / st["attempts"].sum(axis=(0, 1))

    @property
    def round_trips(self) -> np.ndarray:
        """(n_samples,): round trips completed by all walkers of all ladders of each sample."""
        return self._pt.stats()["round_trips"].sum(axis=(1, 2))

    @property
    def walker_at_slot(self) -> np.ndarray:
        """(n_samples, ladders, R): which walker sits at each slot."""
        return self._pt.stats()["walker_at_slot"]

    def spins(self, sample: int, slot: int, ladder: int = 0) -> np.ndarray:
        self._check_sample(sample)
        self._check_slot(slot, ladder)
        return self._pt.get_spins(sample, ladder, slot)

    def energy(self, sample: int, slot: int, ladder: int = 0) -> float:
        self._check_sample(sample)
        self._check_slot(slot, ladder)
        E, _ = self._pt.energies()
        return float(E[sample, ladder, self._pt.stats()["walker_at_slot"][sample, ladder, slot]])


class LatticeTemperingEnsemble(_LatticeTemperingEnsemble):
    """Parallel tempering of many disorder samples of one 2-D lattice at once (K7): sample s is :class:`LatticeTempering` on
    ``couplings[j][s]`` / ``field[s]`` with ``seed=seeds[s]``, bit for bit, but every kernel of a round covers all samples in one
    launch, which is what fills the chip at the lattice sizes a disorder average uses.

    ``couplings=(J_right, J_down)`` of shape ``(S, rows, cols)``, ``field`` ``(S, rows, cols)`` or None; one temperature table for
    all samples; ``seeds`` a length-S sequence, or ``seed`` for ``seeds[s] = seed + s * ladders * R``.  Everything is validated and
    rounded to float32 before any device call.  At most 65535 walkers (S x ladders x R).  No replica cluster moves."""

    def _parse_shape(self, size, periodic):
        self.rows, self.cols = self.shape = tuple(int(n) for n in ((size, size) if np.isscalar(size) else size))
        self.periodic = bool(periodic)

    def _sample_disorder(self, couplings, field):
        return _disorder_arrays(self.rows, self.cols, self.periodic, 1.0, 0.0, "physical", couplings, field)

    def _handle(self):
        return _hip.TemperingEnsemble(self.rows, self.cols, self.periodic, self.n_samples, self.temperatures.size, self.ladders)


class LatticeTemperingEnsemble3D(_LatticeTemperingEnsemble):
    """:class:`LatticeTemperingEnsemble` for the cubic lattices of :class:`IsingModel3D` (K8): sample s is
    :class:`LatticeTempering3D` on its disorder with ``seed=seeds[s]``, bit for bit.  ``couplings=(J_right, J_down, J_layer)`` of
    shape ``(S, depth, rows, cols)``; ``periodic`` a bool or a triple (p_z, p_r, p_c)."""

    def _parse_shape(self, size, periodic):
        self.depth, self.rows, self.cols = self.shape = _shape_3d(size)
        self.periodic = _hip.periodic_axes(periodic)

    def _sample_disorder(self, couplings, field):
        return _tempering_disorder_3d(self.shape, self.periodic, 1.0, 0.0, couplings, field)

    def _handle(self):
        return _hip.TemperingEnsemble3D(self.depth, self.rows, self.cols, self.periodic, self.n_samples, self.temperatures.size,
                                        self.ladders)


def _ensemble_scan(pt, temperatures, n_equilibrate, n_measure, measure_every, swap) -> dict:
    """The body of the ensemble scans on a fresh ensemble ``pt``, closed at the end: per sample the expressions of
    ``_tempering_scan`` on that sample's rows, stacked, then ``ensemble_summary`` of them under ``"average"``."""
    try:
        pt.run(int(n_equilibrate) // int(measure_every), int(measure_every), swap=swap, record=False)
        pt.run(int(n_measure), int(measure_every), swap=swap, record=True)
        hist = pt._pt.history()
        modes = pt.history()["modes"] if pt.correlation else None
        st = pt._pt.stats()
        N, S = pt.n_spins, pt.n_samples
        per_sample = []
        for s in range(S):
            out = {k: np.zeros(len(temperatures)) for k in ("magnetization", "energy", "susceptibility", "specific_heat")}
            out["temperatures"] = temperatures
            Ms = np.ascontiguousarray(hist["M"][:, s, 0].T) / N
            Es = np.ascontiguousarray(hist["E"][:, s, 0].T)
            Qs = np.ascontiguousarray(hist["q"][:, s].T) / N if pt.ladders == 2 else None
            out = _scan_summary(out, N, Ms, Es, Qs)
            if Qs is not None:
                out["overlap_4"] = np.mean(Qs ** 4, axis=1)
            if pt.link_overlap:
                out["link_overlap"] = np.mean(np.ascontiguousarray(hist["q_link"][:, s]), axis=0) / lattice_bond_count(
                    pt._pt.shape, pt._axes_periodic())
            if pt.correlation:
                out["F2"] = np.mean(np.abs(np.ascontiguousarray(modes[s])) ** 2, axis=0)
                out["f2"] = np.mean((Qs if pt.ladders == 2 else Ms) ** 2, axis=1) * float(N) ** 2
                _correlation_summary(out, N, pt._pt.shape, pt._axes_periodic(), out["f2"], out["F2"])
            with np.errstate(divide="ignore", invalid="ignore"):
                out["swap_acceptance"] = st["accepts"][s].sum(axis=0) / st["attempts"][s].sum(axis=0)
            out["round_trips"] = int(st["round_trips"][s].sum())
            del out["temperatures"]
            per_sample.append(out)
        res = {k: np.stack([np.asarray(o[k]) for o in per_sample]) for k in per_sample[0]}
        res["temperatures"] = temperatures
        res["average"] = ensemble_summary(res, N, pt._pt.shape, pt._axes_periodic())
    finally:
        pt.close()
    return res


def _ensemble_scan_args(measure_every, n_equilibrate, replicas, link_overlap):
    if replicas not in (1, 2):
        raise ValueError("replicas must be 1 or 2")
    if link_overlap and replicas != 2:
        raise ValueError("link_overlap=True compares the two replicas at one temperature: it needs replicas=2")
    if int(measure_every) < 1 or int(n_equilibrate) % int(measure_every):
        raise ValueError("n_equilibrate must be a multiple of measure_every")


def tempering_ensemble_scan(size, temperatures, *, couplings, field=None, n_equilibrate: int = 1000, n_measure: int = 50,
                            measure_every: int = 10, periodic: bool = True, seeds=None, seed: Optional[int] = None,
                            initial: str = "up", replicas: int = 1, swap: bool = True, correlation: bool = False,
                            link_overlap: bool = False) -> dict:
    """:func:`tempering_scan` of S disorder samples at once (:class:`LatticeTemperingEnsemble`) and their disorder average.

    Every key of ``tempering_scan(..., couplings=sample s, seed=seeds[s])`` comes back with a leading sample axis, ``(S, R)`` for the
    per-temperature ones, equal to that call's bit for bit; plus per sample ``overlap_4`` (<q^4>) and, with ``correlation``, ``F2``
    and ``f2`` (what the averages of the ratios need).  ``"average"``: :func:`ensemble_summary` of these arrays, the disorder
    averages with their errors over samples.  ``seeds`` / ``seed`` as for the ensemble (default ``seed=0``)."""
    _ensemble_scan_args(measure_every, n_equilibrate, replicas, link_overlap)
    if correlation:
        _check_correlation((bool(periodic),))
    if seeds is None and seed is None:
        seed = 0
    temperatures = np.asarray(temperatures, dtype=float)
    pt = LatticeTemperingEnsemble(size, temperatures, couplings=couplings, field=field, periodic=periodic, seeds=seeds, seed=seed,
                                  initial=initial, ladders=replicas, correlation=correlation, link_overlap=link_overlap)
    return _ensemble_scan(pt, temperatures, n_equilibrate, n_measure, measure_every, swap)


def tempering_ensemble_scan_3d(size, temperatures, *, couplings, field=None, n_equilibrate: int = 1000, n_measure: int = 50,
                               measure_every: int = 10, periodic=True, seeds=None, seed: Optional[int] = None, initial: str = "up",
                               replicas: int = 1, swap: bool = True, correlation: bool = False, link_overlap: bool = False) -> dict:
    """:func:`tempering_ensemble_scan` for cubic lattices: :func:`tempering_scan_3d` of S disorder samples at once
    (:class:`LatticeTemperingEnsemble3D`), per sample and disorder-averaged."""
    _ensemble_scan_args(measure_every, n_equilibrate, replicas, link_overlap)
    if correlation:
        _check_correlation(_hip.periodic_axes(periodic))
    if seeds is None and seed is None:
        seed = 0
    temperatures = np.asarray(temperatures, dtype=float)
    pt = LatticeTemperingEnsemble3D(size, temperatures, couplings=couplings, field=field, periodic=periodic, seeds=seeds, seed=seed,
                                    initial=initial, ladders=replicas, correlation=correlation, link_overlap=link_overlap)
    return _ensemble_scan(pt, temperatures, n_equilibrate, n_measure, measure_every, swap)


# ---------------------------------------------------------------------------------------------------- multispin coding (K9)
MULTISPIN_ROUTES = {"small": _hip.MSC_ROUTE_SMALL, "hbm": _hip.MSC_ROUTE_HBM}


def _multispin_couplings(shape, periodic, couplings, field=None):
    """Validate bimodal couplings of S samples (before any device call): every bond +-1, except the last slice of an open axis,
    which must be 0 as :class:`IsingModel3D` demands.  Returns (S, the three (S, D, R, C) boolean arrays 'J = -1')."""
    if field is not None:
        raise ValueError("field: multispin coding runs the zero-field +-J glass (fields stay on IsingModel3D / the ensembles)")
    for p, n, name in zip(periodic, shape, ("depth", "rows", "cols")):
        if p and (n % 2 or n < 4):
            raise ValueError(f"a periodic axis needs an even length >= 4 ({name} = {n})")
    names = ("J_right", "J_down", "J_layer")
    if couplings is None or len(couplings) not in (2, 3):
        raise ValueError("couplings must be (J_right, J_down, J_layer), or (J_right, J_down) for size=(1, R, C)")
    arrays = [np.asarray(a) for a in couplings]
    if len(arrays) == 2:
        if shape[0] != 1:
            raise ValueError(f"two coupling arrays describe one layer: size must be (1, R, C), got {shape}")
        arrays = [a.reshape((a.shape[0], 1) + a.shape[1:]) if a.ndim == 3 else a for a in arrays]
        arrays.append(np.zeros((arrays[0].shape[0],) + shape, np.float32))
    S = arrays[0].shape[0] if arrays[0].ndim == 4 else -1
    out = []
    # array k holds the bonds along lattice axis 2 - k (J_right: the last axis)
    for k, (a, name) in enumerate(zip(arrays, names)):
        if a.shape != (S,) + shape or S < 1:
            raise ValueError(f"{name} must have shape (n_samples,) + {shape}, got {a.shape}")
        axis = 2 - k
        body = a
        if not periodic[axis]:
            last = np.take(a, -1, axis=axis + 1)
            if np.any(last != 0):
                raise ValueError(f"{name}: open {('depth', 'rows', 'cols')[axis]} axis: the last slice must be 0")
            body = np.delete(a, -1, axis=axis + 1)
        if not np.all((body == 1) | (body == -1)):
            bad = body[(body != 1) & (body != -1)].ravel()[0]
            raise ValueError(f"{name}: multispin coding takes J = +-1 only, got {bad!r} (Gaussian and diluted bonds stay on K7 / K8)")
        out.append(a == -1)
    return S, out


class MultispinGlass3D:
    """S disorder samples of the bimodal (J = +-1, zero field) Edwards-Anderson glass, 64 samples per 64-bit word (K9).

    ``MultispinGlass3D(size, temperatures, couplings=edwards_anderson_samples(size, S, kind="bimodal"), replicas=2)``: every sample
    runs at every temperature, ``replicas`` (1 or 2) independent copies each.  ``size=(1, R, C)`` with ``periodic=(False, p, p)`` takes
    the ``dims=2`` arrays.  Sample s of (slot t, replica a) is, bit for bit, ``IsingModel3D(size, couplings=sample s,
    temperature=T[t], periodic=..., seed=seeds[t][a])`` under ``gibbs_update()``; ``seeds[t][a] = seed + a * n_temps + t`` by default.

    **The samples of one word share their random numbers** (the site's one uniform decides all 64): each sample's chain is exactly
    the single lattice's, but samples 64 w .. 64 w + 63 are correlated with each other, so errors over samples inside one word are not
    independent.  Two replicas of one sample therefore never share a word: they live in different planes with different seeds.

    ``route``: ``"small"`` (planes of at most 8192 sites: the spins stay in LDS for all sweeps of a call, one launch per call) or
    ``"hbm"`` (one launch per half-sweep for all planes); by default the small route where it fits.  No swaps between temperatures here:
    :class:`MultispinTempering3D` adds them.

    ``correlation=True`` (needs a periodic axis) switches on the k_min Fourier modes of the site field f = a b of the two replicas
    of a slot (f = s with one replica): :meth:`fourier_modes`, from the exact integer :meth:`axis_profiles` in the fixed float64
    order of :meth:`IsingModel3D.fourier_modes`, bit for bit what that gives for the sample's two lattices.
    """

    def __init__(self, size, temperatures, *, couplings, periodic=True, replicas: int = 1, seed: Optional[int] = None, seeds=None,
                 initial: str = "random", route: Optional[str] = None, field=None, correlation: bool = False):
        self.depth, self.rows, self.cols = self.shape = _shape_3d(size)
        self.n_spins = self.depth * self.rows * self.cols
        self.periodic = _hip.periodic_axes(periodic)
        self.correlation = bool(correlation)
        if self.correlation:
            _check_correlation(self.periodic)
        self.temperatures = np.asarray(temperatures, dtype=np.float64).ravel()
        if self.temperatures.size < 1 or not np.all(self.temperatures > 0):
            raise ValueError("Temperature must be positive")
        if replicas not in (1, 2):
            raise ValueError("replicas must be 1 or 2")
        if initial not in ("random", "up", "down"):
            raise ValueError("initial must be 'random', 'up' or 'down'")
        if route is not None and route not in MULTISPIN_ROUTES:
            raise ValueError("route must be 'small', 'hbm' or None")
        self.n_samples, packed = _multispin_couplings(self.shape, self.periodic, couplings, field)
        self.replicas = int(replicas)
        nT = self.temperatures.size
        if seeds is not None:
            self.seeds = np.array([[int(x) for x in row] for row in np.asarray(seeds, dtype=object).reshape(nT, self.replicas)], dtype=object)
        else:
            base = int(seed) if seed is not None else (
                int(np.random.randint(0, 2 ** 31 - 1)) | (int(np.random.randint(0, 2 ** 31 - 1)) << 31))
            self.seeds = np.array([[base + a * nT + t for a in range(self.replicas)] for t in range(nT)], dtype=object)
        self.n_bonds = lattice_bond_count(self.shape, self.periodic)
        self.sweep_count = 0
        self._snap_slots, self._snap_taken = 0, set()
        self._before_device()
        self._msc = _hip.MultispinLattice(self.depth, self.rows, self.cols, self.periodic, nT, self.replicas, self.n_samples,
                                          _hip.MSC_ROUTE_AUTO if route is None else MULTISPIN_ROUTES[route])
        self._msc.set_couplings(*(_hip.msc_pack(a) for a in packed))
        self._msc.set_temperatures(self.temperatures)
        self._msc.set_seeds(self.seeds.ravel())
        if self.correlation:
            self._msc.set_correlation([_kmin_tables(n) if p else None for n, p in zip(self.shape, self.periodic)])
        if initial == "random":
            self._msc.randomize()
        else:
            self._msc.fill(1 if initial == "up" else -1)

    def _before_device(self) -> None:
        """What a subclass validates once the samples are counted and the seeds are fixed, before the handle exists."""

    def close(self) -> None:
        self._msc.close()

    @property
    def route(self) -> str:
        return "small" if self._msc.route == _hip.MSC_ROUTE_SMALL else "hbm"

    @property
    def launch_count(self) -> int:
        return self._msc.launch_count()

    def sweep(self, n: int = 1) -> "MultispinGlass3D":
        """n heat-bath sweeps of every sample at every temperature (and of both replicas)."""
        self._msc.sweep(int(n), self.sweep_count)
        self.sweep_count += int(n)
        return self

    def _per_replica(self, x):
        return x if self.replicas == 2 else x[:, 0]

    def energies(self) -> np.ndarray:
        """E = -sum_bonds J s s' per sample, float64 of exact integers: (n_temps, S), or (n_temps, 2, S) with two replicas."""
        unsat = self._msc.measure()[0]
        return self._per_replica((2 * unsat - self.n_bonds).astype(np.float64))

    def magnetizations(self) -> np.ndarray:
        """sum s / N per sample, the shape of :meth:`energies`."""
        return self._per_replica(self._msc.measure()[1] / self.n_spins)

    def overlaps(self) -> np.ndarray:
        """q / N = sum_i a_i b_i / N of the two replicas, (n_temps, S)."""
        if self.replicas != 2:
            raise ValueError("overlaps need replicas=2")
        return self._msc.measure()[2] / self.n_spins

    def link_overlaps(self) -> np.ndarray:
        """q_l = sum_bonds a_i a_j b_i b_j / N_b of the two replicas, (n_temps, S)."""
        if self.replicas != 2:
            raise ValueError("link_overlaps need replicas=2")
        return self._msc.measure()[3] / self.n_bonds

    def axis_profiles(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(P_z, P_r, P_c): int64 (n_temps, S, L_d), the exact sums of a_i b_i of the slot's two replicas (of s_i with one replica)
        over the sites with each coordinate on the axis; each sums to the sample's q N (sum s).  Works without ``correlation``."""
        return self._msc.profiles()

    def fourier_modes(self) -> np.ndarray:
        """complex128 (n_temps, S, 3): F_d = sum_x P_d[x] exp(2 pi i x / L_d) of :meth:`axis_profiles` per axis, NaN on an open
        axis.  Needs ``correlation=True``."""
        if not self.correlation:
            raise ValueError("fourier_modes needs correlation=True")
        return self._msc.modes()

    def spin_array(self) -> np.ndarray:
        """Every spin: int8 (n_temps, replicas, S, D, R, C)."""
        planes = self._msc.get_planes()
        nT, A = planes.shape[:2]
        bits = np.stack([np.stack([_hip.msc_unpack(planes[t, a], self.n_samples) for a in range(A)]) for t in range(nT)])
        return np.where(bits, 1, -1).astype(np.int8)

    def _check_index(self, sample, slot, replica):
        if not 0 <= int(sample) < self.n_samples:
            raise ValueError(f"sample {sample} outside 0 .. {self.n_samples - 1}")
        if not 0 <= int(slot) < self.temperatures.size:
            raise ValueError(f"slot {slot} outside 0 .. {self.temperatures.size - 1}")
        if not 0 <= int(replica) < self.replicas:
            raise ValueError(f"replica {replica} outside 0 .. {self.replicas - 1}")

    def spins(self, sample: int, slot: int, replica: int = 0) -> np.ndarray:
        """int8 (D, R, C) spins of one sample at one temperature slot."""
        self._check_index(sample, slot, replica)
        word = self._msc.get_planes()[int(slot), int(replica), int(sample) // 64]
        return np.where((word >> np.uint64(int(sample) % 64)) & np.uint64(1), 1, -1).astype(np.int8)

    def set_spins(self, sample: int, slot: int, spins, replica: int = 0) -> None:
        self._check_index(sample, slot, replica)
        v = np.asarray(spins).reshape(self.shape)
        if not np.all((v == 1) | (v == -1)):
            raise ValueError("spins must be +1 / -1")
        planes = self._msc.get_planes()
        bit = np.uint64(1) << np.uint64(int(sample) % 64)
        word = planes[int(slot), int(replica), int(sample) // 64]
        planes[int(slot), int(replica), int(sample) // 64] = np.where(v == 1, word | bit, word & ~bit)
        self._msc.set_planes(planes)

    # ---- real space and quenches: C4(r) along the periodic axes, snapshots and two-time correlations (k9_c4, k9_twotime)
    def overlap_correlation(self):
        """(C_z, C_r, C_c): int64 (n_temps, S, L_d / 2 + 1) per periodic axis, ``None`` for an open one:
        C_d[r] = sum_x f_x f_{x + r e_d} over all N sites with wrap-around, r = 0 .. L_d / 2, of the site field f = a b of the slot's
        two replicas (f = s with one replica).  Exact integers; C_d[0] = N."""
        _check_quench_lattice(self.shape, self.periodic)
        return self._msc.c4()

    def _need_slots(self, n: int) -> None:
        if n > self._snap_slots:
            self._msc.snapshot_slots(n)  # the snapshots of the slots that were there stay
            self._snap_slots = n

    def snapshot(self, slot: int = 0) -> None:
        """Store the current planes in ``slot`` (0 .. 7) on the device, for :meth:`two_time`."""
        if not 0 <= int(slot) < _hip.MSC_SNAPSHOT_SLOTS:
            raise ValueError(f"slot {slot} outside 0 .. {_hip.MSC_SNAPSHOT_SLOTS - 1}")
        self._need_slots(int(slot) + 1)
        self._msc.snapshot(int(slot))
        self._snap_taken.add(int(slot))

    def two_time(self, slot: int = 0) -> np.ndarray:
        """sum_x s_x(now) s_x(snapshot in ``slot``) per sample, exact int64 in the shape of :meth:`energies`."""
        if int(slot) not in self._snap_taken:
            raise ValueError(f"slot {slot} holds no snapshot")
        return self._per_replica(self._msc.snapshot_overlap(int(slot)))

    def quench(self, times, waiting_times=()) -> dict:
        """Run ``times[-1]`` sweeps and record, at every ``times[k]`` (strictly ascending sweep counts since the start of the call,
        0: before the first sweep), the measurements, C4 along the periodic axes and, against a snapshot taken at each of
        ``waiting_times`` (a subset of ``times``, at most 8), the two-time correlations; everything is enqueued at once and fetched
        in one transfer.  Returns ``times``, ``energy`` and ``magnetization`` (n_times,) + the shape of :meth:`energies`, with two
        replicas ``overlap`` and ``link_overlap`` (n_times, n_temps, S), ``c4``: the 3-tuple of :meth:`overlap_correlation` with a
        leading time axis, ``waiting_times`` and ``two_time``: float64 (n_wait, n_times) + the shape of :meth:`energies`,
        sum_x s_x(t) s_x(t_w), NaN where t < t_w.  Advances ``sweep_count``; the planes end as after ``sweep(times[-1])``."""
        t, wi = _quench_times(times, waiting_times)
        _check_quench_lattice(self.shape, self.periodic)
        if self.sweep_count + int(t[-1]) > 1 << 31:
            raise ValueError("msc_quench_run: sweep counter overflow")
        self._need_slots(len(wi))
        self._msc.quench_run(t, self.sweep_count, wi)
        self.sweep_count += int(t[-1])
        self._snap_taken.update(range(len(wi)))
        (unsat, ssum, q, ql), c4, tt = self._msc.quench_history()
        per = (lambda x: x) if self.replicas == 2 else (lambda x: x[:, :, 0])
        out = {"times": t.astype(np.int64), "energy": per((2 * unsat - self.n_bonds).astype(np.float64)),
               "magnetization": per(ssum / self.n_spins)}
        if self.replicas == 2:
            out["overlap"] = q / self.n_spins
            out["link_overlap"] = ql / self.n_bonds
        out["c4"] = c4
        out["waiting_times"] = t[wi].astype(np.int64)
        two = tt.astype(np.float64)
        for j, k in enumerate(wi):
            two[j, :k] = np.nan
        out["two_time"] = two if self.replicas == 2 else two[:, :, :, 0]
        return out


def _quench_times(times, waiting_times):
    """Validate a quench's times (before any device call): (times as int32, the indices of the waiting times into them)."""
    raw = np.asarray(times)
    if raw.ndim != 1 or raw.size < 1 or not np.all(raw == np.floor(raw)):
        raise ValueError("times must be a non-empty 1-D sequence of integer sweep counts")
    t = raw.astype(np.int64)
    if t[0] < 0 or np.any(np.diff(t) <= 0) or t[-1] > 1 << 31:
        raise ValueError("times must be strictly ascending, starting at 0 or later")
    w = [int(x) for x in np.asarray(waiting_times).ravel()]
    if len(w) > _hip.MSC_SNAPSHOT_SLOTS:
        raise ValueError(f"at most {_hip.MSC_SNAPSHOT_SLOTS} waiting_times, got {len(w)}")
    if len(set(w)) != len(w) or w != sorted(w):
        raise ValueError("waiting_times must be strictly ascending")
    missing = [x for x in w if x not in set(t.tolist())]
    if missing:
        raise ValueError(f"waiting_times must be a subset of times ({missing[0]} is not among them)")
    where = {int(x): k for k, x in enumerate(t)}
    return t.astype(np.int32), [where[x] for x in w]


def _check_quench_lattice(shape, periodic) -> None:
    if not any(periodic):
        raise ValueError("overlap correlations need at least one periodic axis")
    for n, p in zip(shape, periodic):
        if p and n > _hip.MSC_C4_MAX_AXIS:
            raise ValueError(f"overlap correlations take periodic axes of at most {_hip.MSC_C4_MAX_AXIS} sites, got {n}")


def _xi12(c4, cut: float = 3.0):
    """The coherence-length estimator of :func:`multispin_quench_3d` from per-sample correlators ``c4`` (..., S, r_max + 1):
    (c4_mean, c4_error, xi12, xi12_error, r_cut).  c4_mean and c4_error are the mean and its standard error over the sample axis;
    r_cut (...,) is the last r before c4_mean[r] < cut * c4_error[r] for the first time, or r_max; xi12 = I_2 / I_1 with
    I_k = sum_{r = 0}^{r_cut} r^k c4_mean[r]; its error is the delete-one jackknife over samples with r_cut held fixed."""
    c4 = np.asarray(c4, dtype=np.float64)
    S, R = c4.shape[-2], c4.shape[-1]
    mean = c4.mean(axis=-2)
    err = np.full(mean.shape, np.nan) if S < 2 else np.std(c4, axis=-2, ddof=1) / np.sqrt(S)
    with np.errstate(invalid="ignore"):
        below = mean < float(cut) * err  # NaN errors (one sample) never trigger
    r_cut = np.where(below.any(axis=-1), below.argmax(axis=-1) - 1, R - 1)
    r = np.arange(R, dtype=np.float64)
    keep = r <= r_cut[..., None]

    def ratio(m):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.sum(np.where(keep, r ** 2 * m, 0.0), axis=-1) / np.sum(np.where(keep, r * m, 0.0), axis=-1)

    xi = ratio(mean)
    if S < 2:
        return mean, err, xi, np.full(xi.shape, np.nan), r_cut
    tot = c4.sum(axis=-2)
    th = np.stack([ratio((tot - c4[..., i, :]) / (S - 1)) for i in range(S)])
    return mean, err, xi, np.sqrt((S - 1) / S * np.sum((th - th.mean(axis=0)) ** 2, axis=0)), r_cut


def multispin_quench_3d(size, temperatures, *, couplings, times, waiting_times=(), replicas: int = 2, periodic=True,
                        seed: Optional[int] = None, seeds=None, route: Optional[str] = None, cut: float = 3.0) -> dict:
    """Quench S bimodal samples from T = infinity (``initial="random"``) to every temperature (:class:`MultispinGlass3D`, no swaps)
    and record at ``times`` (sweeps since the quench): :meth:`MultispinGlass3D.quench`'s dict, plus

    * ``c4_mean`` (n_times, n_temps, r_max + 1): C_d[r] / N averaged over the samples and over the periodic axes of the longest
      length among them (r_max = half that length), and ``c4_error``, its standard error over samples;
    * ``xi12`` and ``xi12_error`` (n_times, n_temps): the coherence length I_2 / I_1, I_k = sum_{r = 0}^{r_cut} r^k c4_mean[r],
      r_cut the last r before c4_mean[r] < ``cut`` * c4_error[r] for the first time, or r_max (``r_cut`` holds it); the error is a
      delete-one jackknife over samples with r_cut held fixed.  The sum stops at r_cut: no tail is extrapolated;
    * ``aging`` (n_wait, n_times, n_temps): C(t, t_w) / N averaged over samples and replicas, NaN where t < t_w.

    **The 64 samples of a word share their random numbers, and with ``initial="random"`` they also share their starting
    configuration**: errors over samples within one word are therefore correlated (samples in different words differ in neither)."""
    if replicas not in (1, 2):
        raise ValueError("replicas must be 1 or 2")
    _quench_times(times, waiting_times)
    shape, per = _shape_3d(size), _hip.periodic_axes(periodic)
    _check_quench_lattice(shape, per)
    if seeds is None and seed is None:
        seed = 0
    g = MultispinGlass3D(size, temperatures, couplings=couplings, periodic=periodic, replicas=replicas, seed=seed, seeds=seeds,
                         initial="random", route=route)
    try:
        res = g.quench(times, waiting_times)
    finally:
        g.close()
    longest = max(n for n, p in zip(shape, per) if p)
    axes = [d for d in range(3) if per[d] and shape[d] == longest]
    c4 = np.mean([res["c4"][d] for d in axes], axis=0) / float(g.n_spins)  # (n_times, n_temps, S, r_max + 1)
    res["c4_mean"], res["c4_error"], res["xi12"], res["xi12_error"], res["r_cut"] = _xi12(c4, cut)
    two = res["two_time"] / float(g.n_spins)
    res["aging"] = two.mean(axis=-1) if replicas == 1 else two.mean(axis=(-1, -2))
    res["temperatures"] = np.asarray(temperatures, dtype=float)
    return res


def multispin_scan_3d(size, temperatures, *, couplings, n_equilibrate: int = 1000, n_measure: int = 50, measure_every: int = 1,
                      replicas: int = 2, periodic=True, seed: Optional[int] = None, seeds=None, initial: str = "random",
                      route: Optional[str] = None, correlation: bool = False) -> dict:
    """Equilibrate S bimodal samples at every temperature (:class:`MultispinGlass3D`, no swaps), then take ``n_measure`` measurements
    ``measure_every`` sweeps apart.  Per sample, arrays (S, n_temps) under the keys of :func:`tempering_ensemble_scan_3d`:
    ``energy`` (<E> / N of replica 0), ``magnetization`` (<|m|>) and, with two replicas, ``overlap`` (<|q|>), ``overlap_sq``,
    ``overlap_4`` and ``link_overlap`` (<q_l>); ``"average"``: :func:`ensemble_summary` of them.  The samples of one 64-bit word
    share their random numbers: errors over samples within a word are correlated.

    ``correlation=True`` adds, per sample, ``F2`` (S, n_temps, 3) = <|F_d|^2> of the k_min modes of the overlap field (of the spins
    with one replica; NaN on open axes), ``f2`` (S, n_temps) = <(q N)^2> (<(sum s)^2>), and ``chi_k``, ``xi`` and ``xi_over_L`` from
    them, and to ``"average"`` [chi(k_min)], xi and xi_L / L with their jackknife errors; one synchronisation per measurement."""
    if replicas not in (1, 2):
        raise ValueError("replicas must be 1 or 2")
    if int(measure_every) < 1 or int(n_measure) < 1 or int(n_equilibrate) < 0:
        raise ValueError("measure_every and n_measure must be >= 1, n_equilibrate >= 0")
    temperatures = np.asarray(temperatures, dtype=float)
    if seeds is None and seed is None:
        seed = 0
    g = MultispinGlass3D(size, temperatures, couplings=couplings, periodic=periodic, replicas=replicas, seed=seed, seeds=seeds,
                         initial=initial, route=route, correlation=correlation)
    try:
        g.sweep(int(n_equilibrate))
        N, nb = g.n_spins, g.n_bonds
        acc = {k: [] for k in ("e", "m", "q", "ql", "F")}
        for _ in range(int(n_measure)):
            g.sweep(int(measure_every))
            unsat, ssum, q, ql = g._msc.measure()
            acc["e"].append((2 * unsat[:, 0] - nb) / N)
            acc["m"].append(ssum[:, 0] / N)
            if replicas == 2:
                acc["q"].append(q / N)
                acc["ql"].append(ql / nb)
            if correlation:
                acc["F"].append(g.fourier_modes())
        series = {k: np.stack(v) for k, v in acc.items() if v}  # (n_measure, n_temps, S)
        res = {"energy": series["e"].mean(axis=0).T, "magnetization": np.abs(series["m"]).mean(axis=0).T}
        if replicas == 2:
            res["overlap"] = np.abs(series["q"]).mean(axis=0).T
            res["overlap_sq"] = (series["q"] ** 2).mean(axis=0).T
            res["overlap_4"] = (series["q"] ** 4).mean(axis=0).T
            res["link_overlap"] = series["ql"].mean(axis=0).T
        if correlation:
            _multispin_correlation(res, g, series["F"], series["q"] if replicas == 2 else series["m"])
        res["temperatures"] = temperatures
        res["average"] = ensemble_summary(res, N, g.shape, g.periodic) if correlation else ensemble_summary(res)
    finally:
        g.close()
    return res


def _multispin_correlation(res: dict, g, modes, f) -> None:
    """The per-sample correlation results of the multispin scans from the measurements' modes (n_measure, n_temps, S, 3) and total
    field per site f = q / N (or m) (n_measure, n_temps, S): ``F2``, ``f2``, and ``_correlation_summary``'s ``chi_k``, ``xi`` and
    ``xi_over_L`` of each sample."""
    N = g.n_spins
    res["F2"] = np.moveaxis(np.mean(np.abs(modes) ** 2, axis=0), 1, 0)  # (S, n_temps, 3)
    res["f2"] = np.mean(f ** 2, axis=0).T * float(N) ** 2
    per = [_correlation_summary({}, N, g.shape, g.periodic, f2, F2) for f2, F2 in zip(res["f2"], res["F2"])]
    for key in ("chi_k", "xi", "xi_over_L"):
        res[key] = np.stack([o[key] for o in per])


class MultispinTempering3D(MultispinGlass3D):
    """:class:`MultispinGlass3D` with parallel tempering: every sample (and each of its replicas) swaps between neighbouring
    temperature slots on its own, decided and applied on the device with no host synchronisation inside ``run`` (K9).

    A round is ``swap_interval`` sweeps of every plane, one measurement, one swap pass and the exchange.  The pass runs per sample
    s and per replica a over the pairs i = 0 .. n_temps - 2 in order: with E_x the energy of the configuration now at slot i (the
    one an earlier swap of the same pass moved there, if one did) and E_y that at slot i + 1, it accepts iff
    ``delta = (1/T[i] - 1/T[i+1]) * (E_x - E_y) >= 0 or u < exp(delta)``, u the 53-bit uniform of index i, round counter and
    replica a under the key ``swap_seeds[s]``.  **An accepted pair exchanges the two spin configurations of that sample**;
    temperature, threshold table and sweep seed stay with the slot.  So sample s at slot t is, bit for bit,
    ``IsingModel3D(couplings of s, temperature=T[t], seed=seeds[t][a])`` whose spins are replaced at every accepted swap by those
    of the neighbouring slot.  It is *not* :class:`LatticeTempering3D` bit for bit: there the seed travels with the walker, here it
    stays with the slot.

    The swap uniforms are per sample, unlike the sweep uniforms, which the 64 samples of a word share: swaps decorrelate the
    samples of a word only partially, and errors over samples inside one word remain correlated.

    ``swap_seeds``: one per sample, or ``swap_seed`` for ``swap_seeds[s] = swap_seed + s``; by default
    ``swap_seed = seed + 2 * n_temps`` (``seed``: the first plane's), the first value past the default sweep seeds.
    2 to 256 temperatures.

    ``correlation=True``: every recorded round also records, on the device, the k_min modes of the planes the round's measurement
    saw (``history()["modes"]``); a recording round then takes two more launches."""

    def __init__(self, size, temperatures, *, couplings, periodic=True, replicas: int = 1, seed: Optional[int] = None, seeds=None,
                 initial: str = "random", route: Optional[str] = None, field=None, swap_seed: Optional[int] = None, swap_seeds=None,
                 correlation: bool = False):
        nT = np.asarray(temperatures, dtype=np.float64).size
        if not 2 <= nT <= _hip.MSC_PT_MAX_TEMPS:
            raise ValueError(f"parallel tempering needs 2 to {_hip.MSC_PT_MAX_TEMPS} temperatures, got {nT}")
        if swap_seed is not None and swap_seeds is not None:
            raise ValueError("give either swap_seeds= (one per sample) or swap_seed=, not both")
        self._swap_args = (swap_seed, swap_seeds)
        self.round_count = 0
        self._recorded = 0
        super().__init__(size, temperatures, couplings=couplings, periodic=periodic, replicas=replicas, seed=seed, seeds=seeds,
                         initial=initial, route=route, field=field, correlation=correlation)
        self._msc.pt_enable(self.temperatures)
        self._msc.pt_set_swap_seeds(self.swap_seeds)

    def _before_device(self) -> None:
        swap_seed, swap_seeds = self._swap_args
        S = self.n_samples
        if swap_seeds is None:
            if swap_seed is None:  # the first value past the default sweep seeds
                base = int(self.seeds[0][0]) + 2 * self.temperatures.size
                swap_seeds = [(base + s) % 2 ** 64 for s in range(S)]
            else:
                swap_seeds = [int(swap_seed) + s for s in range(S)]
        swap_seeds = [int(x) for x in np.asarray(swap_seeds, dtype=object).ravel()]
        if len(swap_seeds) != S:
            raise ValueError(f"need one swap seed per sample ({S}), got {len(swap_seeds)}")
        if any(not 0 <= x < 2 ** 64 for x in swap_seeds):
            raise ValueError("swap seeds must fit an unsigned 64-bit integer")
        self.swap_seeds = swap_seeds

    def run(self, n_rounds: int, swap_interval: int = 10, swap: bool = True, record: bool = True):
        """n_rounds rounds of swap_interval sweeps each (0: a measurement and a swap pass alone); with ``record`` returns
        :meth:`history`, else None."""
        n, k = int(n_rounds), int(swap_interval)
        if n < 0:
            raise ValueError("n_rounds must be >= 0")
        if k < 0:
            raise ValueError("swap_interval must be >= 0")
        self._msc.pt_run(n, k, swap, record, self.sweep_count, self.round_count)
        self.sweep_count += n * k
        self.round_count += n
        self._recorded = n if record else 0
        return self.history() if record else None

    def history(self) -> dict:
        """The rounds recorded by the last ``run``, each taken after the round's sweeps and before its swap pass, per slot and
        sample as exact integers scaled like :meth:`energies`, :meth:`magnetizations`, :meth:`overlaps` and :meth:`link_overlaps`:
        ``E`` and ``M`` (n_rounds, n_temps, S), or (n_rounds, n_temps, 2, S) with two replicas, and then also ``q`` and ``q_link``
        (n_rounds, n_temps, S), of the two replicas that sat at the slot in that round.  With ``correlation=True`` also ``modes``:
        complex128 (n_rounds, n_temps, S, 3), the k_min modes of the overlap field of those two replicas (of the spins with one
        replica) per axis, NaN on open axes."""
        unsat, ssum, q, ql = self._msc.pt_history(self._recorded)
        per = (lambda x: x) if self.replicas == 2 else (lambda x: x[:, :, 0])
        out = {"E": per((2 * unsat - self.n_bonds).astype(np.float64)), "M": per(ssum / self.n_spins)}
        if self.replicas == 2:
            out["q"] = q / self.n_spins
            out["q_link"] = ql / self.n_bonds
        if self.correlation:
            out["modes"] = (self._msc.pt_history_modes(self._recorded) if self._recorded else
                            np.zeros((0, self.temperatures.size, self.n_samples, 3), np.complex128))
        return out

    def stats(self) -> dict:
        """The device's counters: ``attempts`` and ``accepts`` (replicas, S, n_temps - 1) per pair, ``label_at_slot`` (replicas, S,
        n_temps): which starting configuration sits at each slot, and per label ``flags`` (0 none, 1 bottom, 2 top) and
        ``round_trips`` (replicas, S, n_temps)."""
        return self._msc.pt_stats()

    def acceptance(self) -> np.ndarray:
        """(S, n_temps - 1): accepted / attempted swaps per adjacent pair of slots of each sample, its replicas pooled."""
        st = self._msc.pt_stats()
        with np.errstate(divide="ignore", invalid="ignore"):
            return st["accepts"].sum(axis=0) / st["attempts"].sum(axis=0)

    def round_trips(self) -> np.ndarray:
        """(S,): round trips (slot 0 -> last slot -> slot 0) completed by all configurations of all replicas of each sample."""
        return self._msc.pt_stats()["round_trips"].sum(axis=(0, 2))

    def label_at_slot(self) -> np.ndarray:
        """(S, replicas, n_temps): which starting configuration of the sample sits at each slot."""
        return np.ascontiguousarray(np.moveaxis(self._msc.pt_stats()["label_at_slot"], 0, 1))

    @property
    def swap_launch_count(self) -> int:
        """Launches of the measurement, plan and exchange kernels by ``run`` (``launch_count``: the sweeps')."""
        return self._msc.pt_launch_count()


def multispin_tempering_scan_3d(size, temperatures, *, couplings, n_equilibrate: int = 1000, n_measure: int = 50,
                                measure_every: int = 10, replicas: int = 2, periodic=True, seed: Optional[int] = None, seeds=None,
                                initial: str = "random", route: Optional[str] = None, swap_interval: Optional[int] = None,
                                swap_seed: Optional[int] = None, correlation: bool = False) -> dict:
    """:func:`multispin_scan_3d` with parallel tempering (:class:`MultispinTempering3D`): rounds of ``swap_interval`` sweeps
    (default: ``measure_every``), each followed by a swap pass; ``n_equilibrate`` sweeps of equilibration, then ``n_measure``
    measurements ``measure_every`` sweeps apart taken from the device's record, one host transfer at the end.  ``n_equilibrate`` and
    ``measure_every`` must be multiples of ``swap_interval``.  Returns :func:`multispin_scan_3d`'s keys plus ``acceptance``
    (S, n_temps - 1) and ``round_trips`` (S,), and ``"average"``: :func:`ensemble_summary` of them.  ``correlation=True`` adds what
    it adds to :func:`multispin_scan_3d`, the modes taken from the device's record in the same one transfer."""
    if replicas not in (1, 2):
        raise ValueError("replicas must be 1 or 2")
    if int(measure_every) < 1 or int(n_measure) < 1 or int(n_equilibrate) < 0:
        raise ValueError("measure_every and n_measure must be >= 1, n_equilibrate >= 0")
    k = int(measure_every) if swap_interval is None else int(swap_interval)
    if k < 1 or int(measure_every) % k or int(n_equilibrate) % k:
        raise ValueError("swap_interval must be >= 1 and divide measure_every and n_equilibrate")
    temperatures = np.asarray(temperatures, dtype=float)
    if seeds is None and seed is None:
        seed = 0
    g = MultispinTempering3D(size, temperatures, couplings=couplings, periodic=periodic, replicas=replicas, seed=seed, seeds=seeds,
                             initial=initial, route=route, swap_seed=swap_seed, correlation=correlation)
    try:
        g.run(int(n_equilibrate) // k, k, record=False)
        stride = int(measure_every) // k
        h = g.run(int(n_measure) * stride, k, record=True)
        rows = {key: v[stride - 1::stride] for key, v in h.items()}  # (n_measure, n_temps, [2,] S)
        N = g.n_spins
        e, m = (rows[key][:, :, 0] if replicas == 2 else rows[key] for key in ("E", "M"))
        res = {"energy": (e / N).mean(axis=0).T, "magnetization": np.abs(m).mean(axis=0).T}
        if replicas == 2:
            res["overlap"] = np.abs(rows["q"]).mean(axis=0).T
            res["overlap_sq"] = (rows["q"] ** 2).mean(axis=0).T
            res["overlap_4"] = (rows["q"] ** 4).mean(axis=0).T
            res["link_overlap"] = rows["q_link"].mean(axis=0).T
        if correlation:
            _multispin_correlation(res, g, rows["modes"], rows["q"] if replicas == 2 else m)
        res["acceptance"] = g.acceptance()
        res["round_trips"] = g.round_trips()
        res["temperatures"] = temperatures
        res["average"] = ensemble_summary(res, N, g.shape, g.periodic) if correlation else ensemble_summary(res)
    finally:
        g.close()
    return res


# ---------------------------------------------------------------------------------------------------- population annealing
POPULATION_WEIGHT_ONE = 1 << 30  # the weight of a step's minimum-energy walker


def _population_schedule(betas, temperatures) -> np.ndarray:
    """The schedule as ascending inverse temperatures, from exactly one of ``betas`` (ascending, betas[0] >= 0) and ``temperatures``
    (descending, ``inf`` allowed first), validated on the host."""
    if (betas is None) == (temperatures is None):
        raise ValueError("give exactly one of betas= (ascending) and temperatures= (descending)")
    if betas is not None:
        b = np.asarray(betas, dtype=float).ravel()
    else:
        T = np.asarray(temperatures, dtype=float).ravel()
        if not np.all(T > 0):  # refuses NaN too
            raise ValueError("Temperature must be positive")
        b = 1.0 / T
    if b.size < 2:
        raise ValueError("population annealing needs at least two inverse temperatures (one step)")
    if not np.all(np.isfinite(b)) or b[0] < 0:
        raise ValueError("betas must be finite and >= 0")
    if not np.all(np.diff(b) > 0):
        raise ValueError("betas must increase (temperatures must decrease) along the schedule")
    return b


def _check_population(population) -> int:
    if isinstance(population, bool) or not isinstance(population, (int, np.integer)) or not 2 <= population <= _hip.POPULATION_MAX:
        raise ValueError(f"population must be an integer in [2, {_hip.POPULATION_MAX}], got {population!r}")
    return int(population)


def population_free_energy(betas, S, E_min, mean_E, population: int, n_spins: int) -> dict:
    """The free-energy estimator of a recorded anneal.  Step j multiplies the partition function by Q_j with
    ``ln Q_j = -db_j E_min_j + ln(S_j / (R 2^30))``; ``ln_Z[k] = N ln 2 + sum_{j <= k} ln Q_j`` when ``betas[0] == 0`` (the uniform
    measure), else the difference ``ln Z(betas[k]) - ln Z(betas[0])``.  ``F = -ln_Z / beta`` and ``entropy = beta <E> + ln_Z`` (NaN
    where beta[0] > 0 leaves only differences; F is NaN at beta = 0)."""
    betas = np.asarray(betas, dtype=float)
    db = np.diff(betas)
    lnQ = -db * np.asarray(E_min, dtype=float) + np.log(np.asarray(S, dtype=float) / (float(population) * POPULATION_WEIGHT_ONE))
    absolute = betas[0] == 0.0
    ln_Z = np.concatenate([[0.0], np.cumsum(lnQ)]) + (n_spins * np.log(2.0) if absolute else 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        F = np.where(betas > 0, -ln_Z / betas, np.nan) if absolute else np.full(betas.size, np.nan)
    entropy = betas * np.asarray(mean_E, dtype=float) + ln_Z if absolute else np.full(betas.size, np.nan)
    return {"betas": betas, "ln_Q": lnQ, "ln_Z": ln_Z, "F": F, "entropy": entropy}


def population_family_stats(parent) -> dict:
    """Families by chaining ``parent`` (n_steps, R) from the first step: walker i of the start founds family i.  Per step (row 0: the
    start) ``rho_t = R sum_f (n_f / R)^2``, ``rho_s = exp(-sum_f (n_f / R) ln(n_f / R))`` (Wang, Machta & Katzgraber 2015) and
    ``families``, the number that survive."""
    parent = np.asarray(parent)
    R = parent.shape[1]
    fam = np.arange(R)
    rho_t, rho_s, alive = [1.0], [float(R)], [R]
    for row in parent:
        fam = fam[row]
        p = np.bincount(fam, minlength=R)
        p = p[p > 0] / float(R)
        rho_t.append(float(R * np.sum(p * p)))
        rho_s.append(float(np.exp(-np.sum(p * np.log(p)))))
        alive.append(int(p.size))
    return {"rho_t": np.array(rho_t), "rho_s": np.array(rho_s), "families": np.array(alive)}


def population_pair_mask(parent) -> np.ndarray:
    """bool (n_steps + 1, P), P = R // 2: whether the walkers of the pair (i, i + P) belong to different families at each recorded
    step (row 0: the start, where every walker is a family), the families chained from ``parent`` (n_steps, R) as
    :func:`population_family_stats` chains them.  Two walkers of one family share an ancestor of the start: they are correlated
    copies, not two replicas, and their overlap is left out of every mean."""
    parent = np.asarray(parent)
    R = parent.shape[1]
    P = R // 2
    fam = np.arange(R)
    rows = [fam[:P] != fam[P:2 * P]]
    for row in parent:
        fam = fam[row]
        rows.append(fam[:P] != fam[P:2 * P])
    return np.array(rows, dtype=bool).reshape(parent.shape[0] + 1, P)


def _masked_mean(x, mask) -> np.ndarray:
    """Row means of x (rows, P, ...) over the pairs with mask (rows, P) set; NaN for a row without one."""
    x = np.asarray(x, dtype=np.float64)
    n = mask.sum(axis=1).astype(np.float64)
    m = mask.reshape(mask.shape + (1,) * (x.ndim - 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(m, x, 0.0).sum(axis=1) / n.reshape((-1,) + (1,) * (x.ndim - 2))


def population_overlap_stats(parent, q, q_link, n_spins: int, n_bonds: int, modes=None, lengths=None, periodic=None) -> dict:
    """Per recorded step, over the pairs (i, i + P) of different families (:func:`population_pair_mask`) only, NaN where there is
    none: ``pairs`` (their number), ``overlap`` (<|q|>), ``overlap_sq`` (<q^2>), ``binder`` (1/2 (3 - <q^4> / <q^2>^2)), with
    q = (sum_i s_i s'_i) / N as in :func:`temperature_scan`, and ``link_overlap`` (<L> / N_b).  With ``modes`` (rows, P, n_axes;
    NaN on open axes), ``lengths`` and ``periodic`` also ``chi_k``, ``xi`` and ``xi_over_L`` of the overlap field."""
    mask = population_pair_mask(parent)
    Q = np.asarray(q, dtype=np.float64) / float(n_spins)
    out = {"pairs": mask.sum(axis=1), "overlap": _masked_mean(np.abs(Q), mask), "overlap_sq": _masked_mean(Q ** 2, mask)}
    with np.errstate(divide="ignore", invalid="ignore"):
        out["binder"] = 0.5 * (3.0 - _masked_mean(Q ** 4, mask) / out["overlap_sq"] ** 2)
    out["link_overlap"] = _masked_mean(np.asarray(q_link, dtype=np.float64), mask) / float(n_bonds)
    if modes is not None:
        F2 = _masked_mean(np.abs(np.asarray(modes)) ** 2, mask)
        _correlation_summary(out, n_spins, lengths, periodic, out["overlap_sq"] * float(n_spins) ** 2, F2)
    return out


def population_overlap_histogram(parent, q, n_spins: int, bins: int = 50) -> dict:
    """P(q) per recorded step: the histogram of q = (sum_i s_i s'_i) / N over the pairs of different families, ``bins`` equal bins
    on [-1, 1], normalised to integrate to 1 (NaN for a step without such a pair).  ``edges`` (bins + 1,), ``P`` (rows, bins),
    ``pairs`` (rows,)."""
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or bins < 1:
        raise ValueError("bins must be an integer >= 1")
    mask = population_pair_mask(parent)
    Q = np.asarray(q, dtype=np.float64) / float(n_spins)
    edges = np.linspace(-1.0, 1.0, int(bins) + 1)
    Pq = np.full((mask.shape[0], int(bins)), np.nan)
    for k, (row, m) in enumerate(zip(Q, mask)):
        if m.any():
            Pq[k] = np.histogram(row[m], bins=edges)[0] / (m.sum() * (2.0 / int(bins)))
    return {"edges": edges, "P": Pq, "pairs": mask.sum(axis=1)}


class _PopulationAnnealing:
    """What :class:`PopulationAnnealing` and :class:`PopulationAnnealing3D` share: everything but the shape and the disorder.  A
    subclass parses its shape, calls ``_check``, validates its disorder into ``self._disorder`` and hands its handle to ``_start``."""

    def _check(self, population, betas, temperatures, sweeps_per_step, initial_sweeps):
        self.population = _check_population(population)
        self.betas = _population_schedule(betas, temperatures)
        if int(sweeps_per_step) < 0 or int(initial_sweeps) < 0:
            raise ValueError("sweeps_per_step and initial_sweeps must be >= 0")
        self.sweeps_per_step, self.initial_sweeps = int(sweeps_per_step), int(initial_sweeps)

    overlap = correlation = False

    def _axes_periodic(self):
        p = self.periodic
        return tuple(p) if isinstance(p, tuple) else (bool(p),) * 2

    def _set_overlap(self, overlap, correlation):
        """Before any device call: keep the flags; the modes belong to the overlap field and need a periodic axis."""
        self.overlap, self.correlation = bool(overlap), bool(correlation)
        if self.correlation:
            if not self.overlap:
                raise ValueError("correlation=True records the k_min modes of the pairs' overlap field: it needs overlap=True")
            _check_correlation(self._axes_periodic())

    def _start(self, pa, seed):
        self._pa = pa
        self.seed = int(seed) if seed is not None else (
            int(np.random.randint(0, 2 ** 31 - 1)) | (int(np.random.randint(0, 2 ** 31 - 1)) << 31))
        pa.set_disorder(*self._disorder)
        pa.set_schedule(self.betas)
        if self.overlap:  # the tables are made here, on the host
            pa.set_overlap(True, [_kmin_tables(n) if per else None for n, per in zip(pa.shape, self._axes_periodic())]
                           if self.correlation else None)
        pa.init(self.seed, self.initial_sweeps)
        self._record = None    # the rows since init while every run recorded, else None
        self._complete = True  # no run since init went unrecorded

    @property
    def n_steps(self) -> int:
        """Steps of the schedule."""
        return self.betas.size - 1

    @property
    def step_count(self) -> int:
        return self._pa.step_count

    @property
    def sweep_count(self) -> int:
        return self._pa.sweep_count

    def run(self, n_steps: Optional[int] = None, resample: bool = True, record: bool = True):
        """``n_steps`` further steps of the schedule (default: all that are left); with ``record`` returns ``history()``."""
        left = self.n_steps - self.step_count
        n = left if n_steps is None else int(n_steps)
        if not 0 <= n <= left:
            raise ValueError(f"n_steps = {n} runs past the schedule ({left} of {self.n_steps} steps left)")
        self._pa.run(n, self.sweeps_per_step, resample, record)
        if not record:
            self._complete, self._record = False, None
            return None
        h = self._history_rows()
        if self._complete:
            if self._record is None:
                self._record = h
            else:  # row 0 of a later run repeats the last row of the one before
                r = self._record
                self._record = {k: np.concatenate([r[k], h[k][1:] if k in ("E", "M", "q", "q_link", "modes") else h[k]]) for k in h}
        return self.history()

    def history(self) -> dict:
        """Every step since the start, if every run recorded (else the last run's steps): ``E`` (float64), ``M`` (int64 sum of spins)
        as (n + 1, R) arrays by walker index, row 0 the start; ``W`` (uint32 weights), ``parent`` (int32) (n, R); ``S``, ``U``
        (uint64), ``E_min`` (n,); ``resampled`` (n,) bool.  Steps taken with ``resample=False`` have ``parent`` = identity and zeros in
        ``W``, ``S``, ``U``, ``E_min``.  With ``overlap=True`` also, per pair (i, i + R // 2): ``q`` (int64 sum_i s_i s'_i) and ``q_link``
        (int64 L; q_l = L / N_b) as (n + 1, R // 2) and, with ``correlation=True``, ``modes``: complex128 (n + 1, R // 2, n_axes), the
        k_min mode of each axis profile of the pair's overlap field (NaN on an open axis)."""
        if self._complete and self._record is not None:
            return dict(self._record)
        return self._history_rows()

    def _history_rows(self) -> dict:
        """The handle's rows of the last run, the modes spread over all axes."""
        h = self._pa.history()
        if "modes" in h:
            per = np.asarray(self._axes_periodic(), dtype=bool)
            modes = np.full(h["modes"].shape[:2] + (per.size,), complex(np.nan, np.nan), dtype=np.complex128)
            modes[:, :, per] = h["modes"]
            h["modes"] = modes
        return h

    def _full_record(self, what):
        if not (self._complete and self._record is not None):
            raise ValueError(f"{what} needs the record of every step since the start: run with record=True throughout")
        return self._record

    def free_energy(self) -> dict:
        """``ln_Z``, ``F`` and ``entropy`` at every recorded beta (:func:`population_free_energy`); needs resampled steps."""
        r = self._full_record("free_energy")
        if not np.all(r["resampled"]):
            raise ValueError("free_energy needs resampled steps (run(resample=True))")
        k = r["S"].size
        return population_free_energy(self.betas[:k + 1], r["S"], r["E_min"], r["E"].mean(axis=1), self.population, self.n_spins)

    def observables(self) -> dict:
        """Population means per recorded beta: ``energy`` (<E>), ``energy_sq``, ``abs_magnetization`` (<|M|> / N),
        ``magnetization_sq`` (<M^2> / N^2), with ``betas``."""
        r = self._full_record("observables")
        m = r["M"] / float(self.n_spins)
        return {"betas": self.betas[:r["E"].shape[0]], "energy": r["E"].mean(axis=1), "energy_sq": (r["E"] ** 2).mean(axis=1),
                "abs_magnetization": np.abs(m).mean(axis=1), "magnetization_sq": (m ** 2).mean(axis=1)}

    def family_stats(self) -> dict:
        """``rho_t``, ``rho_s`` and ``families`` per recorded beta (:func:`population_family_stats`)."""
        return population_family_stats(self._full_record("family_stats")["parent"])

    def _overlap_record(self, what):
        r = self._full_record(what)
        if "q" not in r:
            raise ValueError(f"{what} needs the overlaps of the walker pairs: create the population with overlap=True")
        return r

    def overlap_stats(self) -> dict:
        """Per recorded beta, over the pairs (i, i + R // 2) whose walkers belong to different families only (NaN where there is
        none): ``pairs``, ``overlap``, ``overlap_sq``, ``binder``, ``link_overlap`` and, with ``correlation=True``, ``chi_k``, ``xi``
        and ``xi_over_L`` of the overlap field (:func:`population_overlap_stats`), with ``betas``."""
        r = self._overlap_record("overlap_stats")
        shape = self._pa.shape
        out = population_overlap_stats(r["parent"], r["q"], r["q_link"], self.n_spins, lattice_bond_count(shape, self._axes_periodic()),
                                       r.get("modes"), shape, self._axes_periodic())
        out["betas"] = self.betas[:r["q"].shape[0]]
        return out

    def overlap_histogram(self, bins: int = 50) -> dict:
        """P(q) per recorded beta over the pairs of different families (:func:`population_overlap_histogram`), with ``betas``."""
        r = self._overlap_record("overlap_histogram")
        out = population_overlap_histogram(r["parent"], r["q"], self.n_spins, bins)
        out["betas"] = self.betas[:r["q"].shape[0]]
        return out

    def spins(self, i: int) -> np.ndarray:
        """Spins of walker ``i``, in the lattice's shape."""
        if not 0 <= i < self.population:
            raise ValueError(f"walker {i} out of range (population {self.population})")
        return self._pa.get_spins(i)

    def energies(self) -> np.ndarray:
        """Every walker's energy now (the device's fixed-order float64 sums)."""
        return self._pa.energies()[0]


class PopulationAnnealing(_PopulationAnnealing):
    """Population annealing of a disordered lattice on the GPU (K7, physical mode; Hukushima & Iba 2003, Machta 2010).

    ``population`` walkers (2 ... 65535) share one quenched disorder, ``couplings=(J_right, J_down)`` and ``field`` as for
    :class:`IsingModel2D` or the uniform ``coupling`` / ``external_field``, validated and rounded to float32 before any device call.
    The schedule is exactly one of ``betas`` (ascending, first >= 0) and ``temperatures`` (descending, ``inf`` allowed first).
    Walker i is ``IsingModel2D(seed=seed + i)``: same Philox key, initial draw and sweep counter; a first beta of 0 makes that draw
    the equilibrium start, a larger one takes ``initial_sweeps`` sweeps there.  Each step reweights the population from beta[k-1]
    to beta[k] by systematic resampling at fixed size with 30-bit integer weights (walkers lighter than 2^-31 of the step's
    heaviest are dropped), copies the planes of the walkers that multiply over those that die, sweeps every walker
    ``sweeps_per_step`` times at 1 / beta[k] and computes every energy, all on the device without a host synchronisation.
    ``run(resample=False)`` anneals the walkers independently (the single lattices, bit for bit).  From the record:
    ``free_energy()``, ``observables()`` and ``family_stats()``.  Fixed population, one GPU, fixed schedule.

    ``overlap=True`` also records, for the start and after every step, the spin overlap ``q`` and the link overlap ``q_link`` of the
    walker pairs (i, i + population // 2), and ``correlation=True`` (needs ``overlap=True`` and a periodic axis) the k_min modes of
    each pair's overlap field, all on the device within the same run.  Two walkers are two replicas of the disorder only while they
    descend from different walkers of the start: ``overlap_stats()`` and ``overlap_histogram()`` average over those pairs alone.
    One partner per walker, a fixed pairing, P(q) binned on the host.
    """

    def __init__(self, size, population, *, betas=None, temperatures=None, couplings=None, field=None, coupling: float = 1.0,
                 external_field: float = 0.0, periodic: bool = True, seed: Optional[int] = None, sweeps_per_step: int = 10,
                 initial_sweeps: int = 0, overlap: bool = False, correlation: bool = False):
        self.rows, self.cols = (size, size) if np.isscalar(size) else tuple(size)
        self.n_spins = self.rows * self.cols
        self._check(population, betas, temperatures, sweeps_per_step, initial_sweeps)
        self.periodic = bool(periodic)
        self._set_overlap(overlap, correlation)
        self._disorder = _disorder_arrays(self.rows, self.cols, self.periodic, float(coupling), float(external_field), "physical",
                                          couplings, field)
        self._start(_hip.PopulationLattice(self.rows, self.cols, self.periodic, self.population), seed)


class PopulationAnnealing3D(_PopulationAnnealing):
    """Population annealing of a disordered cubic lattice on the GPU (K8): :class:`PopulationAnnealing` for the lattices of
    :class:`IsingModel3D` (``couplings=(J_right, J_down, J_layer)``; ``periodic`` a bool or a triple (p_z, p_r, p_c)).  Walker i is
    ``IsingModel3D(seed=seed + i)``."""

    def __init__(self, size, population, *, betas=None, temperatures=None, couplings=None, field=None, coupling: float = 1.0,
                 external_field: float = 0.0, periodic=True, seed: Optional[int] = None, sweeps_per_step: int = 10,
                 initial_sweeps: int = 0, overlap: bool = False, correlation: bool = False):
        self.depth, self.rows, self.cols = self.shape = _shape_3d(size)
        self.n_spins = self.depth * self.rows * self.cols
        self._check(population, betas, temperatures, sweeps_per_step, initial_sweeps)
        self.periodic = _hip.periodic_axes(periodic)
        self._set_overlap(overlap, correlation)
        self._disorder = _tempering_disorder_3d(self.shape, self.periodic, float(coupling), float(external_field), couplings, field)
        self._start(_hip.PopulationLattice3D(self.depth, self.rows, self.cols, self.periodic, self.population), seed)


def _population_scan(pa) -> dict:
    """The body of the population scans on a fresh population ``pa``, closed at the end: the whole schedule, then
    temperature_scan's keys per temperature from the population at that temperature, plus ``ln_Z``, ``rho_t`` and ``rho_s``."""
    try:
        h = pa.run()
        N = pa.n_spins
        with np.errstate(divide="ignore"):
            temperatures = 1.0 / pa.betas
        out = {k: np.zeros(temperatures.size) for k in ("magnetization", "energy", "susceptibility", "specific_heat")}
        out["temperatures"] = temperatures
        out = _scan_summary(out, N, h["M"] / float(N), h["E"])
        out["betas"] = pa.betas.copy()
        out["ln_Z"] = pa.free_energy()["ln_Z"]
        fam = pa.family_stats()
        out["rho_t"], out["rho_s"] = fam["rho_t"], fam["rho_s"]
        if pa.overlap:
            out.update({k: v for k, v in pa.overlap_stats().items() if k != "betas"})
    finally:
        pa._pa.close()
    return out


def population_annealing_scan(size, population, *, betas=None, temperatures=None, coupling: float = 1.0, couplings=None, field=None,
                              external_field: float = 0.0, periodic: bool = True, seed: int = 0, sweeps_per_step: int = 10,
                              initial_sweeps: int = 0, overlap: bool = False, correlation: bool = False) -> dict:
    """:func:`temperature_scan`'s keys (``temperatures``, ``magnetization``, ``energy``, ``susceptibility``, ``specific_heat``) per
    temperature of the schedule, as population means of one :class:`PopulationAnnealing` run, plus ``betas``, ``ln_Z`` (differences
    from the first beta unless it is 0), ``rho_t`` and ``rho_s``.  ``overlap=True`` (and ``correlation=True``) add the keys of
    :meth:`PopulationAnnealing.overlap_stats`."""
    return _population_scan(PopulationAnnealing(size, population, betas=betas, temperatures=temperatures, couplings=couplings,
                                                field=field, coupling=coupling, external_field=external_field, periodic=periodic,
                                                seed=seed, sweeps_per_step=sweeps_per_step, initial_sweeps=initial_sweeps,
                                                overlap=overlap, correlation=correlation))


def population_annealing_scan_3d(size, population, *, betas=None, temperatures=None, coupling: float = 1.0, couplings=None,
                                 field=None, external_field: float = 0.0, periodic=True, seed: int = 0, sweeps_per_step: int = 10,
                                 initial_sweeps: int = 0, overlap: bool = False, correlation: bool = False) -> dict:
    """:func:`population_annealing_scan` for the cubic lattices of :class:`PopulationAnnealing3D`."""
    return _population_scan(PopulationAnnealing3D(size, population, betas=betas, temperatures=temperatures, couplings=couplings,
                                                  field=field, coupling=coupling, external_field=external_field, periodic=periodic,
                                                  seed=seed, sweeps_per_step=sweeps_per_step, initial_sweeps=initial_sweeps,
                                                  overlap=overlap, correlation=correlation))

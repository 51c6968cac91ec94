"""Parallel tempering and multi-start annealing of a sparse coupling graph: many walkers per launch (K5 walker batches).

No reference counterpart: the reference's ``parallel_tempering`` (tsu/gibbs.py:238-338) loops over replicas of a dense matrix on the
host.  Here ``ladders`` ladders of ``len(temperatures)`` walkers share the CSR graph of one handle; the half-sweeps, the fixed-order
energies and the swap passes are batched launches (include/tsu_hip_sparse_batch.h, DESIGN.md sections 3 and 5).  The swap rule is the
lattice ladders' detailed-balance rule, not the reference's inverted ``E_b - E_a``.
"""
import numpy as np

from .. import _hip

_INITIAL = {"random": 0, "ones": 1, "zeros": -1}


def _check_temperatures(temperatures):
    T = np.asarray(temperatures, dtype=np.float64).reshape(-1)
    if T.size < 1:
        raise ValueError("GraphTempering needs at least one temperature")
    if T.size > _hip.BATCH_MAX_TEMPS:
        raise ValueError(f"GraphTempering holds at most {_hip.BATCH_MAX_TEMPS} temperatures, got {T.size}")
    if not (np.all(np.isfinite(T)) and np.all(T > 0)):
        raise ValueError("Temperature must be positive")
    return T


class GraphTempering:
    """``ladders`` tempering ladders over ``temperatures`` on the graph of ``coupling`` (a ``scipy.sparse`` matrix or an ndarray of
    bit couplings, diagonal allowed) with biases ``bias``.

    Walker ``g = ladder * n_temps + w`` starts at slot ``w``.  A sweep of walker ``g`` is ``SparseSystem.sweep(T_of_its_slot, 1, seed,
    sweep, replica=g)`` bit for bit; the energies are fixed-order sums (the same bits on every run).  Equal temperatures are legal:
    with ``swap=False`` they give independent chains.  ``initial``: ``"random"``, ``"zeros"`` or ``"ones"``.  ``track_best=True`` keeps
    every walker's lowest-energy state on the device (see :meth:`best`)."""

    def __init__(self, coupling, temperatures, bias=None, ladders=1, seed=0, initial="random", track_best=False):
        from ..graph import canonical_csr, color_graph
        if not hasattr(coupling, "shape"):
            coupling = np.asarray(coupling)
        shape = coupling.shape
        if len(shape) != 2 or shape[0] != shape[1]:
            raise ValueError("Coupling matrix must be square")
        T = _check_temperatures(temperatures)
        ladders = int(ladders)
        if ladders < 1:
            raise ValueError(f"GraphTempering needs at least one ladder, got {ladders}")
        if ladders * T.size > _hip.BATCH_MAX_WALKERS:
            raise ValueError(f"GraphTempering holds at most {_hip.BATCH_MAX_WALKERS} walkers, got {ladders} x {T.size}")
        if initial not in _INITIAL:
            raise ValueError(f"initial must be one of {sorted(_INITIAL)}, got {initial!r}")
        n = int(shape[0])
        b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float64).reshape(n)
        A = canonical_csr(coupling)
        offsets, order = color_graph(A)
        self.n, self.n_temps, self.ladders, self.seed = n, int(T.size), ladders, int(seed)
        self.temperatures = T.copy()
        self.n_colors = len(offsets) - 1
        self.csr, self.color_offsets, self.order = A, offsets, order  # the graph as the device holds it (site order, visiting order)
        self._graph = _hip.SparseSystem(A.indptr, A.indices, A.data, b, offsets, order)
        self._batch = _hip.SparseBatch(self._graph, self.n_temps, ladders)
        self._batch.set_temperatures(T)
        self._batch.init(self.seed, _INITIAL[initial])
        if track_best:
            self._batch.track_best(True)
        self.tracks_best = bool(track_best)

    def close(self):
        if getattr(self, "_batch", None) is not None:
            self._batch.close()
            self._batch = None
        if getattr(self, "_graph", None) is not None:
            self._graph.close()
            self._graph = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------ runs
    def run(self, n_rounds, swap_interval=10, swap=True, record=True):
        """``n_rounds`` rounds of ``swap_interval`` sweeps of every walker followed by one swap pass per ladder (``swap``) and one
        history row (``record``).  Nothing waits for the device."""
        self._batch.run(n_rounds, swap_interval, swap, record)
        return self

    def set_temperatures(self, temperatures):
        """Slot -> temperature for the runs that follow (enqueued; the walkers keep their slots)."""
        T = _check_temperatures(temperatures)
        if T.size != self.n_temps:
            raise ValueError(f"expected {self.n_temps} temperatures, got {T.size}")
        self._batch.set_temperatures(T)
        self.temperatures = T.copy()

    def anneal(self, schedule, sweeps_per_step=1):
        """One temperature per step (every walker of every ladder takes it) or a row of ``n_temps`` temperatures per step; each step
        sets the temperatures and runs one round of ``sweeps_per_step`` sweeps without swaps.  No synchronisation inside: with
        ``track_best`` this is a multi-start simulated annealing whose best states stay on the device."""
        S = np.asarray(schedule, dtype=np.float64)
        if S.ndim == 1:
            S = np.repeat(S[:, None], self.n_temps, axis=1)
        if S.ndim != 2 or S.shape[1] != self.n_temps:
            raise ValueError(f"schedule must have shape (steps,) or (steps, {self.n_temps}), got {np.shape(schedule)}")
        if not (np.all(np.isfinite(S)) and np.all(S > 0)):
            raise ValueError("Temperature must be positive")
        if int(sweeps_per_step) < 1:
            raise ValueError("sweeps_per_step must be >= 1")
        for row in S:
            self._batch.set_temperatures(row)
            self._batch.run(1, int(sweeps_per_step), False, False)
        if len(S):
            self.temperatures = S[-1].copy()
        return self

    # ------------------------------------------------------------------ readers
    def history(self, ladder=0):
        """``E``, ``M``, ``walker`` of the last recording run, each (rounds, n_temps), by slot."""
        E, M, W = self._batch.history()
        return {"E": E[:, ladder], "M": M[:, ladder], "walker": W[:, ladder]}

    def acceptance(self):
        """Accepted / attempted swaps per adjacent pair, (ladders, n_temps - 1); NaN where nothing was attempted."""
        s = self._batch.stats()
        att = s["attempts"].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(att > 0, s["accepts"] / att, np.nan)

    def swap_counts(self):
        s = self._batch.stats()
        return s["attempts"], s["accepts"]

    def round_trips(self):
        return self._batch.stats()["round_trips"]

    def walker_at_slot(self):
        return self._batch.stats()["walker_at_slot"]

    @property
    def sweep_count(self):
        return self._batch.stats()["sweep_count"]

    def state(self, slot, ladder=0):
        """The bits {0,1} (site order) of the walker now at ``slot``."""
        return self._batch.get_state(ladder, slot)

    def set_state(self, slot, bits, ladder=0):
        self._batch.set_state(ladder, slot, bits)

    def energies(self):
        """Energy of the walker at each slot now, (ladders, n_temps)."""
        E, _ = self._batch.energies()
        was = self.walker_at_slot()
        return np.take_along_axis(E, was.astype(np.int64), axis=1)

    def energy(self, slot, ladder=0):
        return float(self.energies()[ladder, slot])

    def best(self):
        """``(bits, energy)`` of the lowest-energy state any walker has held at an energy pass of a tracked run (the first minimum in
        walker order)."""
        if not self.tracks_best:
            raise ValueError("best() needs track_best=True")
        found = None
        for k in range(self.ladders):
            e, _, _ = self._batch.best(k, bits=False)
            if found is None or e < found[0]:
                found = (e, k)
        e, bits, _ = self._batch.best(found[1], bits=True)
        return bits, e

    def plan(self):
        """The route of the next run (``"colour"`` / ``"small"``), walkers per thread, padded walkers, launches per sweep, the further
        launches of a round that swaps or records, and the energy segments."""
        p = self._batch.plan()
        p["route"] = "small" if p["route"] == _hip.BATCH_ROUTE_SMALL else "colour"
        return p

    @property
    def launch_count(self):
        return self._batch.launch_count()

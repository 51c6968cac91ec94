"""K5 walker batches without a GPU: the contract's twin (tests/helpers/sparse_batch_twin.py) samples the exact Boltzmann distribution
with and without swaps, its fixed-order energy against the oracle's, the argument validation that happens before a handle is made,
and the C ABI's header / ctypes agreement."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
from scipy import stats

from oracle import oracle as ora
from test_sparse_cpu import random_graph  # (tests/ is on sys.path: rootdir conftest, prepend import mode)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_spec = importlib.util.spec_from_file_location("sparse_batch_twin", os.path.join(HERE, "helpers", "sparse_batch_twin.py"))
twin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(twin)

NEW_SYMBOLS = ["tsu_sparse_batch_" + name for name in (
    "create", "destroy", "set_temperatures", "init", "set_state", "get_state", "run", "history", "stats", "energies", "track_best",
    "best", "plan", "launch_count")]


# ---------------------------------------------------------------- equilibrium against exact enumeration
def _tau_int(x):
    """Integrated autocorrelation time of a series, summed up to the first non-positive autocorrelation (>= 0.5)."""
    x = np.asarray(x, dtype=np.float64) - np.mean(x)
    var = float(np.mean(x * x))
    if var == 0.0:
        return 0.5
    tau = 0.5
    for lag in range(1, x.size // 10):
        rho = float(np.mean(x[:-lag] * x[lag:])) / var
        if rho <= 0.0:
            break
        tau += rho
    return tau


@pytest.mark.parametrize("swap", [True, False])
def test_cold_slot_samples_the_exact_boltzmann_distribution(swap):
    """random_graph(8, 0.4) without a diagonal (the heat-bath conditional is exact) plus biases, three temperatures: the histogram of
    the cold slot's state over the 256 states against exact enumeration, chi-square on the states with expected count >= 5 (the others
    pooled), the series thinned by twice its measured integrated autocorrelation time.  p > 1e-4 at the first seed tried; swaps off
    is the control (the same chains without exchange)."""
    from tsu.graph import color_graph
    n, seed, rounds = 8, 1, 12000
    A = random_graph(n, 0.4, seed, self_loops=False)
    bias = np.random.default_rng(seed).normal(size=n) * 0.5
    temps = [1.0, 1.7, 2.8]
    _, order = color_graph(A)
    all_states = ((np.arange(256)[:, None] >> np.arange(n)) & 1).astype(np.int8)
    table = np.array([twin.fixed_order_energy(s, A, bias, order) for s in all_states])
    weights = 1 << np.arange(n)

    def energies(j, b):
        return table[[int(s @ weights) for s in b.states]]

    b = twin.Batch(A, bias, order, temps, ladders=1, seed=77)
    b.run(200, 1, swap=swap, record=False, energies=energies)  # burn-in
    idx = np.empty(rounds, dtype=np.int64)
    for t in range(rounds):
        b.run(1, 1, swap=swap, record=False, energies=energies)
        idx[t] = int(b.state_at(0) @ weights)
    if swap:
        assert b.accepts.sum() > 0.2 * b.attempts.sum() and b.attempts.sum() == 2 * (rounds + 200)
    else:
        assert b.attempts.sum() == 0
    tau = _tau_int(table[idx])
    thin = max(1, int(np.ceil(2.0 * tau)))
    kept = idx[::thin]
    p_exact = np.exp(-(table - table.min()) / temps[0])
    p_exact /= p_exact.sum()
    expected = p_exact * kept.size
    counts = np.bincount(kept, minlength=256).astype(np.float64)
    big = expected >= 5.0
    obs = np.append(counts[big], counts[~big].sum())
    exp = np.append(expected[big], expected[~big].sum())
    if exp[-1] < 5.0:  # the pooled tail joins the smallest kept bin
        j = int(np.argmin(exp[:-1]))
        obs[j] += obs[-1]
        exp[j] += exp[-1]
        obs, exp = obs[:-1], exp[:-1]
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    p = float(stats.chi2.sf(chi2, obs.size - 1))
    print(f"swap={swap}: tau_int={tau:.2f} thin={thin} samples={kept.size} bins={obs.size} chi2={chi2:.1f} p={p:.3g}")
    assert big.sum() >= 20 and kept.size >= 2000
    assert p > 1e-4


# ---------------------------------------------------------------- the fixed-order energy
def _masked_dyadic(n, density, seed):
    J, b, _ = ora.dyadic_system(n, seed)
    rng = np.random.default_rng(seed)
    keep = np.triu(rng.random((n, n)) < density)
    keep = keep | keep.T
    return sp.csr_matrix(J * keep), b


@pytest.mark.parametrize("n", [1, 7, 300, 1500, 70000])
def test_fixed_order_energy_against_the_oracle(n):
    """Exact on dyadic couplings (every summation order gives the same number), within rel 1e-12 on Gaussian couplings; n = 70000
    has two energy segments."""
    from tsu.graph import canonical_csr, color_graph
    rng = np.random.default_rng(n)
    if n <= 1500:
        Jd, bd = _masked_dyadic(n, min(1.0, 6.0 / n), n)
        A = canonical_csr(Jd)
        assert ora.energy_is_exact(A.toarray(), bd)
        _, order = color_graph(A)
        for _ in range(3):
            s = rng.integers(0, 2, size=n).astype(np.int8)
            assert twin.fixed_order_energy(s, A, bd, order) == ora.sparse_energy(s, A.indptr, A.indices, A.data, bd)
    G = random_graph(n, 3.0 / n, n) if n > 1 else canonical_csr(sp.csr_matrix(np.array([[0.7]])))
    bias = rng.normal(size=n)
    _, order = color_graph(G)
    for b_ in (bias, None):
        s = rng.integers(0, 2, size=n).astype(np.int8)
        assert twin.fixed_order_energy(s, G, b_, order) == pytest.approx(ora.sparse_energy(s, G.indptr, G.indices, G.data, b_), rel=1e-12, abs=1e-9)


def test_twin_fields_are_the_sequential_row_sums():
    A = random_graph(50, 0.2, 5)
    s = np.random.default_rng(5).integers(0, 2, size=50).astype(np.int8)
    F = twin.fields(s, A)
    for i in range(50):
        h = 0.0
        for e in range(A.indptr[i], A.indptr[i + 1]):
            h += A.data[e] * float(s[A.indices[e]])
        assert F[i] == h


# ---------------------------------------------------------------- validation before the device is touched
def test_validation_happens_before_a_handle_is_made(monkeypatch):
    from tsu import _hip
    from tsu.gibbs import GibbsConfig, GibbsSampler
    from tsu.models import GraphTempering

    def no_device(*a, **k):
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(_hip, "SparseSystem", no_device)
    monkeypatch.setattr(_hip, "SparseBatch", no_device)
    monkeypatch.setattr(_hip.Context, "default", classmethod(no_device))
    A = random_graph(12, 0.3, 2)
    with pytest.raises(ValueError, match="square"):
        GraphTempering(sp.csr_matrix((3, 4)), [1.0, 2.0])
    with pytest.raises(ValueError, match="square"):
        GraphTempering(np.zeros((3, 4)), [1.0, 2.0])
    with pytest.raises(ValueError, match="at least one temperature"):
        GraphTempering(A, [])
    with pytest.raises(ValueError, match="at most 256"):
        GraphTempering(A, np.linspace(1.0, 2.0, 257))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="Temperature must be positive"):
            GraphTempering(A, [1.0, bad])
    with pytest.raises(ValueError, match="at most 65535 walkers"):
        GraphTempering(A, np.linspace(1.0, 2.0, 256), ladders=256)
    with pytest.raises(ValueError, match="initial"):
        GraphTempering(A, [1.0, 2.0], initial="up")
    with pytest.raises(ValueError, match="philox"):
        GibbsSampler(GibbsConfig(), rng="numpy").parallel_tempering(A, [1.0, 2.0], n_samples=2)
    with pytest.raises(ValueError, match="sequential"):
        GibbsSampler(GibbsConfig(update_order="random"), seed=1).parallel_tempering(A, [1.0, 2.0], n_samples=2)
    with pytest.raises(ValueError, match="square"):
        GibbsSampler(GibbsConfig(), seed=1).parallel_tempering(sp.csr_matrix((3, 4)), [1.0, 2.0], n_samples=2)


def test_python_surface():
    import inspect
    import tsu
    from tsu import models
    from tsu.models import graph_tempering
    assert tsu.GraphTempering is models.GraphTempering is graph_tempering.GraphTempering
    assert "GraphTempering" in tsu.__all__ and "GraphTempering" in models.__all__
    assert list(inspect.signature(models.GraphTempering).parameters) == ["coupling", "temperatures", "bias", "ladders", "seed", "initial",
                                                                         "track_best"]
    for attr in ("run", "history", "acceptance", "round_trips", "walker_at_slot", "sweep_count", "state", "energy", "energies", "best",
                 "anneal", "plan", "launch_count", "close"):
        assert hasattr(models.GraphTempering, attr), attr


# ---------------------------------------------------------------- header and bindings
def test_header_and_ctypes_prototypes_agree():
    """The entry points are declared in include/tsu_hip_sparse_batch.h, which tsu_hip.h includes after tsu_hip_ensemble.h, exported by
    the library, and prototyped one to one in _hip.SPARSE_BATCH_SIGNATURES (which load_library declares); SIGNATURES is unchanged."""
    from tsu import _hip
    with open(os.path.join(ROOT, "include", "tsu_hip.h")) as f:
        top = f.read()
    assert re.search(r'^#include "tsu_hip_sparse_batch.h"', top, flags=re.M)
    assert top.index('#include "tsu_hip_ensemble.h"') < top.index('#include "tsu_hip_sparse_batch.h"')
    with open(os.path.join(ROOT, "include", "tsu_hip_sparse_batch.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tsu_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_hip.SPARSE_BATCH_SIGNATURES)
    lib = _hip.load_library()
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW_SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_hip.SPARSE_BATCH_SIGNATURES[name][1]), name
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == _hip.SPARSE_BATCH_SIGNATURES[name][1]
    older = (set(_hip.SIGNATURES) | set(_hip.CLUSTER3D_SIGNATURES) | set(_hip.CORRELATION_SIGNATURES) | set(_hip.POPULATION_SIGNATURES)
             | set(_hip.OVERLAP_SIGNATURES) | set(_hip.ENSEMBLE_SIGNATURES))
    assert not older & set(NEW_SYMBOLS)
    top_plain = re.sub(r"/\*.*?\*/", "", top, flags=re.S)
    assert sorted(_hip.SIGNATURES) == sorted(set(re.findall(r"\b(tsu_[a-z0-9_]+)\s*\(", top_plain)))
    build = open(os.path.join(ROOT, "tsu-emulator_amd", "csrc", "build.sh")).read()
    for header_name in ("sparse.h", "sparse_batch_dev.h", "tsu_hip_sparse_batch.h"):
        assert header_name in build, header_name

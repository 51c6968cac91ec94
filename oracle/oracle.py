"""CPU ORACLE -- test infrastructure, NOT product code.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module.
The shipped package (tsu-emulator_amd/) never does; its ops fail loudly without the HIP library.

Contents
  * NumPy restatements of the reference algorithms, in the reference's own visiting order, with
    the random draws passed in (so NumPy's legacy MT19937 stream can be replayed bit for bit):
      ref_sigmoid, ref_gibbs_sweep, ref_sample_boltzmann, ref_compute_energy,
      ref_langevin_step, ref_numerical_gradient, ref_sample_from_energy,
      ref_grid_coupling, ref_bit_coupling, ref_bit_bias
    Each cites the reference lines it follows; all are pinned by tests/golden/g*.npz, which were
    produced by running the unmodified reference (tests/golden/make_golden.py).
  * ctypes bindings of oracle/tsu_oracle.c: the same restatements in C plus the "device-order"
    twins (checkerboard + Philox) that define the bit-exact contract for the HIP kernels.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "tsu_oracle.c")
_LIB = os.path.join(_HERE, "_build", "libtsu_oracle.so")

MODE_PHYSICAL = 0
MODE_COMPAT = 1


def build(force=False):
    """Compile oracle/tsu_oracle.c with gcc into oracle/_build/ (idempotent)."""
    if not force and os.path.exists(_LIB) and os.path.getmtime(_LIB) >= os.path.getmtime(_SRC):
        return _LIB
    os.makedirs(os.path.dirname(_LIB), exist_ok=True)
    tmp = _LIB + ".tmp%d" % os.getpid()
    subprocess.check_call(["gcc", "-O2", "-fno-fast-math", "-ffp-contract=off", "-shared", "-fPIC",
                           "-o", tmp, _SRC, "-lm"])
    os.replace(tmp, _LIB)
    return _LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.ora_sigmoid.restype = C.c_double
        _lib.ora_sigmoid.argtypes = [C.c_double]
        _lib.ora_dense_energy.restype = C.c_double
        _lib.ora_dense_uniform.restype = C.c_double
        _lib.ora_sparse_energy.restype = C.c_double
        _lib.ora_dense_uniform.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32]
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


# ============================================================================ reference order (NumPy)

def ref_sigmoid(x):
    """tsu/gibbs.py:61-77 -- hard clamp beyond +-20, else 1/(1+exp(-x))."""
    if x > 20:
        return 1.0
    elif x < -20:
        return 0.0
    return 1.0 / (1.0 + np.exp(-x))


def ref_gibbs_sweep(state, coupling, bias, T, uniforms, order=None):
    """tsu/gibbs.py:128-162 with :97-100 and :124-126 inlined.

    uniforms: (n_sweeps, n) doubles consumed in visiting order; order: None or (n_sweeps, n).
    Returns a new state array of the input dtype (the input is not modified, gibbs.py:150).
    """
    state = state.copy()
    n = len(state)
    uniforms = np.asarray(uniforms, dtype=np.float64).reshape(-1, n)
    for s in range(uniforms.shape[0]):
        idx = range(n) if order is None else order[s]
        for k, i in enumerate(idx):
            h = np.dot(coupling[i, :], state)
            if bias is not None:
                h += bias[i]
            prob = ref_sigmoid(float(h) / T)
            state[i] = 1 if uniforms[s, k] < prob else 0
    return state


def ref_sample_boltzmann(coupling, bias, T, burnin, n_sweeps, n_samples, init, uniforms, order=None):
    """tsu/gibbs.py:164-213 given the initial state and the replayed draws.

    uniforms / order: (burnin + n_sweeps*n_samples, n).  Returns (n_samples, n) int64.
    """
    n = coupling.shape[0]
    if coupling.shape != (n, n):
        raise ValueError("Coupling matrix must be square")
    state = np.asarray(init).copy()
    o = None if order is None else order[:burnin]
    state = ref_gibbs_sweep(state, coupling, bias, T, uniforms[:burnin].reshape(-1, n), o) if burnin else state
    samples = np.zeros((n_samples, n), dtype=int)
    pos = burnin
    for k in range(n_samples):
        o = None if order is None else order[pos:pos + n_sweeps]
        state = ref_gibbs_sweep(state, coupling, bias, T, uniforms[pos:pos + n_sweeps], o)
        pos += n_sweeps
        samples[k] = state
    return samples


def ref_compute_energy(state, coupling, bias=None):
    """tsu/gibbs.py:215-236."""
    e = -0.5 * state.dot(coupling).dot(state)
    if bias is not None:
        e -= bias.dot(state)
    return float(e)


def ref_grid_coupling(rows, cols, J, periodic):
    """tsu/models/ising.py:343-361 -- dense coupling matrix of the square lattice.

    Bonds are SET (not added): on a periodic dimension of size 2 the wrap bond coincides with the
    direct bond; on a periodic dimension of size 1 the wrap bond is a self-coupling J_ii.
    """
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


def ref_bit_coupling(J):
    """tsu/models/ising.py:138."""
    return 4 * J


def ref_bit_bias(J, h, mode=MODE_COMPAT):
    """tsu/models/ising.py:148 (compat, as shipped) or the corrected conversion (physical)."""
    if mode == MODE_COMPAT:
        return -2 * h + 2 * np.sum(J, axis=1)
    return 2 * h - 2 * np.sum(J, axis=1)


def ref_langevin_step(x, grad, noise, T, dt, friction):
    """tsu/core.py:64-80 with np.random.randn(*x.shape) replaced by `noise`."""
    drift = -grad * dt / friction
    noise_scale = np.sqrt(2 * T * dt / friction)
    diffusion = noise_scale * noise
    return x + drift + diffusion


def ref_numerical_gradient(energy_fn, x, eps=1e-5):
    """tsu/core.py:82-98."""
    x = np.atleast_1d(x)
    grad = np.zeros_like(x)
    for i in range(len(x)):
        xp = x.copy()
        xp[i] += eps
        xm = x.copy()
        xm[i] -= eps
        grad[i] = (float(energy_fn(xp)) - float(energy_fn(xm))) / (2 * eps)
    return grad


def ref_sample_from_energy(energy_fn, x_init, n_samples, T, dt, friction, n_burnin, n_steps, draws):
    """tsu/core.py:135-162 with every np.random.randn draw taken from `draws` in order.

    Returns (samples (n_samples, d), trajectory list of the sampling-phase states).
    """
    draws = iter(np.asarray(draws))
    x = np.atleast_1d(x_init).copy()
    samples, traj = [], []
    for s in range(n_samples):
        if s > 0:
            x = x_init + 0.1 * next(draws)
        for _ in range(n_burnin):
            x = ref_langevin_step(x, ref_numerical_gradient(energy_fn, x), next(draws), T, dt, friction)
        for _ in range(n_steps):
            x = ref_langevin_step(x, ref_numerical_gradient(energy_fn, x), next(draws), T, dt, friction)
            traj.append(x.copy())
        samples.append(x.copy())
    return np.array(samples), traj


# ============================================================================ C restatements (ctypes)

def philox4x32_10(ctr, key):
    ctr = np.ascontiguousarray(ctr, dtype=np.uint32)
    key = np.ascontiguousarray(key, dtype=np.uint32)
    out = np.zeros(4, dtype=np.uint32)
    lib().ora_philox4x32_10(_p(ctr, C.c_uint32), _p(key, C.c_uint32), _p(out, C.c_uint32))
    return out


def c_sigmoid(x):
    return lib().ora_sigmoid(float(x))


def c_dense_sweep_replay(state, J, bias, T, uniforms, order=None):
    st = np.ascontiguousarray(state, dtype=np.int64).copy()
    n = st.size
    Jc = np.ascontiguousarray(J, dtype=np.float64)
    u = np.ascontiguousarray(uniforms, dtype=np.float64).reshape(-1, n)
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float64)
    o = None if order is None else np.ascontiguousarray(order, dtype=np.int64).reshape(-1, n)
    lib().ora_dense_sweep_replay(_p(st, C.c_int64), _p(Jc, C.c_double), None if b is None else _p(b, C.c_double),
                                 C.c_int(n), C.c_double(T), C.c_int(u.shape[0]),
                                 None if o is None else _p(o, C.c_int64), _p(u, C.c_double))
    return st


def c_dense_energy(state, J, bias=None):
    st = np.ascontiguousarray(state, dtype=np.int64)
    Jc = np.ascontiguousarray(J, dtype=np.float64)
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float64)
    return lib().ora_dense_energy(_p(st, C.c_int64), _p(Jc, C.c_double), None if b is None else _p(b, C.c_double),
                                  C.c_int(st.size))


def c_langevin_step_f64(x, grad, noise, T, dt, friction):
    xx = np.ascontiguousarray(x, dtype=np.float64).copy()
    g = np.ascontiguousarray(grad, dtype=np.float64)
    nz = np.ascontiguousarray(noise, dtype=np.float64)
    lib().ora_langevin_step_f64(_p(xx, C.c_double), _p(g, C.c_double), _p(nz, C.c_double), C.c_int(xx.size),
                                C.c_double(T), C.c_double(dt), C.c_double(friction))
    return xx


# ---------------------------------------------------------------------------- device-order twins

def ising2d_thresholds(J, h, T, mode=MODE_PHYSICAL):
    """table[deg*5+up] (uint64, 0..2^32): see ora_ising2d_thresholds."""
    t = np.zeros(25, dtype=np.uint64)
    lib().ora_ising2d_thresholds(C.c_double(J), C.c_double(h), C.c_double(T), C.c_int(mode), _p(t, C.c_uint64))
    return t


def ising2d_thresholds_numpy(J, h, T, mode=MODE_PHYSICAL):
    """The same table from the NumPy restatement of _sigmoid (cross-check of the C helper)."""
    t = np.zeros(25, dtype=np.uint64)
    for deg in range(5):
        for up in range(deg + 1):
            bias = (-2.0 * h + 2.0 * J * deg) if mode == MODE_COMPAT else (2.0 * h - 2.0 * J * deg)
            p = ref_sigmoid((4.0 * J * up + bias) / T)
            t[deg * 5 + up] = int(np.floor(p * 4294967296.0 + 0.5))
    return t


def ising2d_randomize(rows, cols, seed, replica=0, row0=0):
    s = np.zeros((rows, cols), dtype=np.int8)
    lib().ora_ising2d_randomize(_p(s, C.c_int8), C.c_int(rows), C.c_int(cols), C.c_int64(row0),
                                C.c_uint64(seed), C.c_uint32(replica))
    return s


def ising2d_sweep(spins, periodic, table, n_sweeps, seed, sweep0=0, replica=0, plain=False):
    """n_sweeps checkerboard heat-bath sweeps; returns a new (rows, cols) int8 array."""
    s = np.ascontiguousarray(spins, dtype=np.int8).copy()
    assert s.ndim == 2
    t = np.ascontiguousarray(table, dtype=np.uint64)
    assert t.size == 25
    fn = lib().ora_ising2d_sweep_plain if plain else lib().ora_ising2d_sweep
    fn(_p(s, C.c_int8), C.c_int(s.shape[0]), C.c_int(s.shape[1]), C.c_int(int(bool(periodic))), _p(t, C.c_uint64),
       C.c_int(n_sweeps), C.c_uint64(seed), C.c_uint32(sweep0), C.c_uint32(replica))
    return s


def ising2d_observables(spins, periodic):
    s = np.ascontiguousarray(spins, dtype=np.int8)
    a, b = C.c_int64(0), C.c_int64(0)
    lib().ora_ising2d_observables(_p(s, C.c_int8), C.c_int(s.shape[0]), C.c_int(s.shape[1]),
                                  C.c_int(int(bool(periodic))), C.byref(a), C.byref(b))
    return a.value, b.value


def dense_uniform(i, t, seed, replica=0):
    return lib().ora_dense_uniform(int(i), int(t), int(seed), int(replica))


def dense_sweep_philox(state, J, bias, T, n_sweeps, seed, sweep0=0, replica=0, order=None):
    st = np.ascontiguousarray(state, dtype=np.int8).copy()
    n = st.size
    Jc = np.ascontiguousarray(J, dtype=np.float64)
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float64)
    o = None if order is None else np.ascontiguousarray(order, dtype=np.int64).reshape(n_sweeps, n)
    lib().ora_dense_sweep_philox(_p(st, C.c_int8), _p(Jc, C.c_double), None if b is None else _p(b, C.c_double),
                                 C.c_int(n), C.c_double(T), C.c_int(n_sweeps),
                                 None if o is None else _p(o, C.c_int64), C.c_uint64(seed), C.c_uint32(sweep0),
                                 C.c_uint32(replica))
    return st


def sparse_sweep_philox(state, row_ptr, col, val, bias, T, n_sweeps, seed, sweep0=0, replica=0, order=None):
    """K5 twin: sequential heat-bath sweeps on a CSR graph in the visiting order ``order`` (n sites, the same every sweep).
    Reference loop: tsu/gibbs.py:128-162; field incl. the diagonal entry: gibbs.py:97."""
    st = np.ascontiguousarray(state, dtype=np.int8).copy()
    n = st.size
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
    ci = np.ascontiguousarray(col, dtype=np.int32)
    va = np.ascontiguousarray(val, dtype=np.float64)
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float64)
    o = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    lib().ora_sparse_sweep_philox(_p(st, C.c_int8), _p(rp, C.c_int64), _p(ci, C.c_int32), _p(va, C.c_double),
                                  None if b is None else _p(b, C.c_double), C.c_int(n), C.c_double(T), C.c_int(n_sweeps),
                                  None if o is None else _p(o, C.c_int32), C.c_uint64(seed), C.c_uint32(sweep0), C.c_uint32(replica))
    return st


def sparse_energy(state, row_ptr, col, val, bias):
    st = np.ascontiguousarray(state, dtype=np.int8)
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
    ci = np.ascontiguousarray(col, dtype=np.int32)
    va = np.ascontiguousarray(val, dtype=np.float64)
    b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float64)
    return float(lib().ora_sparse_energy(_p(st, C.c_int8), _p(rp, C.c_int64), _p(ci, C.c_int32), _p(va, C.c_double),
                                         None if b is None else _p(b, C.c_double), C.c_int(st.size)))


TAG_LANGEVIN = 3
TAG_LANGEVIN_RESTART = 5


def langevin_normals_f32(q, chain, step, seed, tag=TAG_LANGEVIN):
    out = np.zeros(4, dtype=np.float32)
    lib().ora_langevin_normals_f32(C.c_uint32(q), C.c_uint32(chain), C.c_uint32(step), C.c_uint32(tag),
                                   C.c_uint64(seed), _p(out, C.c_float))
    return out


def langevin_quadratic_f32(x, k, mu, n_steps, dt, gamma, T, seed, step0=0, chain0=0, trajectory=False):
    """x: (n_chains, dim) float32.  Returns x_final or (x_final, traj (n_steps, n_chains, dim))."""
    xx = np.ascontiguousarray(x, dtype=np.float32).copy()
    if xx.ndim == 1:
        xx = xx[None, :]
    n_chains, dim = xx.shape
    kk = np.ascontiguousarray(np.broadcast_to(np.asarray(k, dtype=np.float32), (dim,)))
    mm = np.ascontiguousarray(np.broadcast_to(np.asarray(mu, dtype=np.float32), (dim,)))
    traj = np.zeros((n_steps, n_chains, dim), dtype=np.float32) if trajectory else None
    lib().ora_langevin_quadratic_f32(_p(xx, C.c_float), _p(kk, C.c_float), _p(mm, C.c_float), C.c_int(n_chains),
                                     C.c_int(dim), C.c_int(n_steps), C.c_float(dt), C.c_float(gamma), C.c_float(T),
                                     C.c_uint64(seed), C.c_uint32(step0), C.c_uint32(chain0),
                                     None if traj is None else _p(traj, C.c_float))
    return (xx, traj) if trajectory else xx


def langevin_coupled_f32(x, A, b, n_steps, dt, gamma, T, seed, step0=0, chain0=0, trajectory=False):
    """Langevin steps on E = 1/2 x^T A x + b^T x (A symmetric (dim, dim)); x: (n_chains, dim) float32.  Returns x_final or
    (x_final, traj (n_steps, n_chains, dim))."""
    xx = np.ascontiguousarray(x, dtype=np.float32).copy()
    if xx.ndim == 1:
        xx = xx[None, :]
    n_chains, dim = xx.shape
    aa = np.ascontiguousarray(A, dtype=np.float32).reshape(dim, dim)
    bb = None if b is None else np.ascontiguousarray(np.broadcast_to(np.asarray(b, dtype=np.float32), (dim,)))
    traj = np.zeros((n_steps, n_chains, dim), dtype=np.float32) if trajectory else None
    lib().ora_langevin_coupled_f32(_p(xx, C.c_float), _p(aa, C.c_float), None if bb is None else _p(bb, C.c_float), C.c_int(n_chains),
                                   C.c_int(dim), C.c_int(n_steps), C.c_float(dt), C.c_float(gamma), C.c_float(T), C.c_uint64(seed),
                                   C.c_uint32(step0), C.c_uint32(chain0), None if traj is None else _p(traj, C.c_float))
    return (xx, traj) if trajectory else xx


def ising2d_site_uniforms(rows, cols, hs, seed, replica=0):
    """(rows, cols) uint32: the uniform each site uses in half-sweep hs = 2*sweep + colour."""
    out = np.zeros((rows, cols), dtype=np.uint32)
    lib().ora_ising2d_site_uniforms(_p(out, C.c_uint32), C.c_int(rows), C.c_int(cols), C.c_uint32(hs),
                                    C.c_uint64(seed), C.c_uint32(replica))
    return out


def ising2d_sweep_window(block, row_global0, total_rows, periodic, table, n_sweeps, seed, sweep0=0, replica=0):
    """Sweeps on a window of rows of a larger lattice (see ora_ising2d_sweep_window); returns a new array."""
    s = np.ascontiguousarray(block, dtype=np.int8).copy()
    t = np.ascontiguousarray(table, dtype=np.uint64)
    lib().ora_ising2d_sweep_window(_p(s, C.c_int8), C.c_int(s.shape[0]), C.c_int(s.shape[1]), C.c_int64(row_global0),
                                   C.c_int64(total_rows), C.c_int(int(bool(periodic))), _p(t, C.c_uint64), C.c_int(n_sweeps),
                                   C.c_uint64(seed), C.c_uint32(sweep0), C.c_uint32(replica))
    return s


# ============================================================================ near-tie chains for the dense decision rule
# The dense kernels decide u < sigmoid(h/T) as x > logit(u) and hand the close calls to the reference's float64 expression:
# inside 1e-9 (1 + |logit|) of the logit and 1e-9 of the +-20 clamp (k2_block, k2_pipe, k2_coop, k2_own), or inside a float32
# band of 1e-4 (1 + |logit|) and 1e-3 of the clamp (k2_small, k2_small_replicas, k2_wg).  Random draws land there about once per
# 1e9 decisions; the generators below put them there on purpose, on systems whose fields are exact in any summation order.

U53 = 2.0 ** -53
BAND_EXACT = 1e-9   # |x - logit(u)| <= BAND_EXACT (1 + |logit(u)|): the large kernels' float64 fallback
BAND_FLOAT = 1e-4   # |x - logit(u)| <= BAND_FLOAT (1 + |logit(u)|): the one-wave / one-workgroup kernels' fallback
CLAMP_BAND_FLOAT = 1e-3
# clamp ladder (class D): x = 2 b at T = 0.5, one value per ladder site
LADDER_X = (20.0, -20.0, 20.0 + 2.0 ** -40, -20.0 - 2.0 ** -40, 20.0 - 2.0 ** -40, -20.0 + 2.0 ** -40, 20.0 + 5e-4, -20.0 - 5e-4,
            20.0 - 5e-4, -20.0 + 5e-4, 20.0 + 2e-3, -20.0 - 2e-3, 20.0 - 2e-3, -20.0 + 2e-3, 25.0, -25.0)
EXTREME_U = (0.0, U53, 1.0 - U53)


def logit(u):
    return math.log(u) - math.log1p(-u) if 0.0 < u < 1.0 else (-math.inf if u <= 0.0 else math.inf)


def _sig(x):
    """ora_sigmoid in Python floats (math.exp is the C library's exp, as in tsu_oracle.c)."""
    if x > 20.0:
        return 1.0
    if x < -20.0:
        return 0.0
    return 1.0 / (1.0 + math.exp(-x))


def ladder_u(x):
    """Class D: the uniform for a clamp-ladder site at x, chosen where the clamped and the unclamped sigmoid disagree (or, just
    inside the clamp, where only the unclamped value is right)."""
    if abs(x) >= 25.0:
        return 1.0 - U53 if x > 0 else U53
    return 1.0 - 2.0 ** -30 if x > 0 else 2.0 ** -30


def dyadic_system(n, seed, sym=True, bias=True, ladder=0, diag=True, mmax=3, rounding=0):
    """A dense system on the grid 2^-K, K = 4 + ceil(log2 sqrt n): J_ij = m_ij 2^-K with integers |m| <= mmax (nonzero diagonal),
    b_i = m_i 2^-K.  Every field J[i,:].s + b_i is exact in float64 and the couplings are exact in float32, so the device's field
    and the oracle's are the same number in any summation order.  The first `ladder` sites have a zero row (their field is their
    bias: the clamp ladder, x = 2 b at T = 0.5) and keep their column; their biases are LADDER_X / 2 (cycled), off the grid.  The
    next `rounding` sites are built the same way with x from rounding_sites (class F at T = 0.5).
    Returns (J float64 (n, n), b float64 (n,) or None, K)."""
    rng = np.random.default_rng(seed)
    K = 4 + int(math.ceil(math.log2(math.sqrt(max(n, 1)))))
    m = rng.integers(-mmax, mmax + 1, size=(n, n))
    if sym:
        m = np.triu(m) + np.triu(m, 1).T
    if diag:
        d = rng.integers(1, mmax + 1, size=n) * rng.choice([-1, 1], size=n)
        m[np.arange(n), np.arange(n)] = d
    J = m.astype(np.float64) * 2.0 ** -K
    b = rng.integers(-4 * mmax, 4 * mmax + 1, size=n).astype(np.float64) * 2.0 ** -K if (bias or ladder or rounding) else None
    if ladder or rounding:
        if b is None:
            b = np.zeros(n)
        xs = [LADDER_X[i % len(LADDER_X)] for i in range(ladder)] + rounding_sites(rounding)
        for i, x in enumerate(xs[:n]):
            J[i, :] = 0.0
            b[i] = x / 2.0
    return J, b, K


def energy_is_exact(J, b):
    """True when -1/2 s^T J s - b^T s is exact in float64 for every 0/1 state in any summation order: J and b on one grid 2^-K
    and sum |terms| < 2^(53 - K)."""
    vals = np.abs(np.concatenate([np.ravel(J), [] if b is None else np.ravel(b)]))
    vals = vals[vals > 0]
    if vals.size == 0:
        return True
    K = 0
    while K < 60 and not np.all(vals * 2.0 ** K == np.floor(vals * 2.0 ** K)):
        K += 1
    return K < 60 and float(vals.sum()) < 2.0 ** (52 - K)


def _place(cls, x, o, rng):
    """The uniform for a visit at x with outcome o (1: u < sigmoid(x)) in placement class cls, or None where the class cannot
    land at this x.  Multiples of 2^-53 only."""
    p = _sig(x)
    if cls == "A":  # 64 ... 1024 units of 2^-53 from p: inside every band
        if abs(x) > 12.0:
            return None
        kmax = min(1024, int(0.4 * BAND_EXACT * (1.0 + abs(x)) * p * (1.0 - p) / U53))
        if kmax < 64:
            return None
        k = int(rng.integers(64, kmax + 1))
        u = (math.floor(p / U53) - k) * U53 if o else (math.ceil(p / U53) + k) * U53
        return u if 0.0 < u < 1.0 else None
    if cls in "BC":  # 3e-9 (1 + |x|): between the two bands; 2e-4 (1 + |x|): just outside the float band
        if abs(x) > 15.0:
            return None
        dx = (3e-9 if cls == "B" else 2e-4) * (1.0 + abs(x))
        u = round(_sig(x - dx if o else x + dx) / U53) * U53
        return u if 0.0 < u < 1.0 else None
    if cls == "E":
        return EXTREME_U[int(rng.integers(0, 3))]
    if cls == "F":
        return rounding_u(x)
    return None


def rounding_u(x):
    """Class F: for 10 <= x <= 18 the reference's p = 1 / (1 + exp(-x)) is the exact sigmoid rounded twice (1 + e to 2^-52, then
    the division), an error of up to ~1.5 units of 2^-53 in p, i.e. up to ~1e-8 in x: inside the float64 band.  Returns the
    multiple of 2^-53 on which the reference's expression and the exact comparison x > logit(u) disagree, or None where there is
    none with room to spare or where p would change if exp(-x) were off by up to 16 ulp."""
    if not 10.0 <= x <= 18.0:
        return None
    e = math.exp(-x)
    p = 1.0 / (1.0 + e)
    if any(1.0 / (1.0 + e * (1.0 + k * 2.0 ** -52)) != p for k in range(-16, 17)):
        return None
    d = (p - 1.0) + e / (1.0 + e)  # p minus the exact sigmoid (p - 1 is exact; e / (1 + e) = 1 - sigmoid to ~1e-16 relative)
    if d < -0.25 * U53:
        return p  # reference: u < p is false -> 0; exact: u < sigmoid(x) -> 1
    if d > 1.25 * U53:
        return p - U53  # reference -> 1; exact -> 0
    return None


def rounding_sites(count, step=2.0 ** -7):
    """`count` values of x on [10, 18) (multiples of `step`) where class F has a uniform (rounding_u), half of them where the
    reference's outcome is 0 and half where it is 1: for the zero-row sites at T = 0.5."""
    out = {0: [], 1: []}
    for j in range(int(8.0 / step)):
        x = 10.0 + ((j * 97) % int(8.0 / step)) * step
        u = rounding_u(x)
        if u is not None:
            out[1 if u < _sig(x) else 0].append(x)
    half = (count + 1) // 2
    return (out[0][:half] + out[1][:count - half])[:count]


def classify(x, u):
    """Where a decision at x with uniform u lies: 'A' inside the float64 band, 'B' outside it and inside the float band, 'C' outside
    both bands, with |x - logit(u)| itself; the clamp bands are reported apart ('D': within 1e-3 of +-20)."""
    lg = logit(u)
    dist = abs(x - lg)
    if abs(abs(x) - 20.0) < CLAMP_BAND_FLOAT:
        return "D", dist
    if dist <= BAND_EXACT * (1.0 + abs(lg)):
        return "A", dist
    if dist <= BAND_FLOAT * (1.0 + abs(lg)):
        return "B", dist
    return "C", dist


def dense_tie_chain(J, b, temps, order=None, rng=None, classes="ABCDEF", state=None, ladder=0):
    """Replayed-uniform near-tie chain: the reference's sequential loop (gibbs.py:128-162) with one temperature per sweep
    (temps, length = sweeps) and an optional visiting order ((sweeps, n)), where every draw is placed on purpose.

    At each visit the exact field h (one row dot product: J must be dyadic, see dyadic_system, so any order gives the oracle's
    number) gives x = h / T;
    a target outcome and a placement class are drawn and the uniform chosen (classes: 'A' within 64 ... 1024 units of 2^-53 of p,
    'B' 3e-9 (1 + |x|) from the logit, 'C' 2e-4 (1 + |x|), 'D' the clamp ladder (sites < `ladder` at T = 0.5), 'E' u in {0, 2^-53,
    1 - 2^-53}, 'F' where the reference's rounded sigmoid and the exact comparison disagree (10 <= x <= 18, see rounding_u; the
    zero-row sites after the ladder sit there at T = 0.5); 'R' an ordinary draw where no requested class fits).
    Returns dict(uniforms (sweeps, n) in visiting order, states (sweeps + 1, n) int8, cls (sweeps, n) str by position,
    x (sweeps, n) float64 by position)."""
    rng = np.random.default_rng(0) if rng is None else rng
    J = np.asarray(J, dtype=np.float64)
    n = J.shape[0]
    temps = [float(t) for t in temps]
    S = len(temps)
    s = (rng.integers(0, 2, size=n) if state is None else np.asarray(state)).astype(np.int8).copy()
    sf = s.astype(np.float64)
    bb = None if b is None else np.asarray(b, dtype=np.float64)
    ordinary = [c for c in classes if c in "ABCEF"]
    out_u = np.zeros((S, n))
    out_x = np.zeros((S, n))
    out_c = np.full((S, n), "R", dtype="<U1")
    states = np.zeros((S + 1, n), dtype=np.int8)
    states[0] = s
    for t in range(S):
        T = temps[t]
        idx = range(n) if order is None else [int(v) for v in order[t]]
        picks = rng.integers(0, 1 << 30, size=n)
        outs = rng.integers(0, 2, size=n)
        for k, i in enumerate(idx):
            x = (float(J[i] @ sf) + (0.0 if bb is None else float(bb[i]))) / T
            o = int(outs[k])
            u, c = None, "R"
            if i < ladder and T == 0.5 and "D" in classes:
                u, c = ladder_u(x), "D"
            elif "F" in classes and rounding_u(x) is not None:  # (rare but for the zero-row sites after the ladder)
                u, c = rounding_u(x), "F"
            elif ordinary:
                first = int(picks[k]) % len(ordinary)
                for j in range(len(ordinary)):
                    c = ordinary[(first + j) % len(ordinary)]
                    u = _place(c, x, o, rng)
                    if u is not None:
                        break
            if u is None:
                u, c = float(rng.random()), "R"
            new = 1 if u < _sig(x) else 0
            out_u[t, k], out_x[t, k], out_c[t, k] = u, x, c
            s[i] = sf[i] = new
        states[t + 1] = s
    return {"uniforms": out_u, "states": states, "cls": out_c, "x": out_x}


def dense_tie_bias(J, T, order, seed, sweep0, replica, state, rng=None, classes="ABC"):
    """Philox-mode near ties: a bias b (non-dyadic) such that the FIRST sweep of a call at temperature T from `state` (visiting
    order `order` (n,) or None; uniforms dense_uniform(site, sweep0, seed, replica)) puts every site near its own uniform: within
    class-A distance (64 ... 1024 units of 2^-53 of p, i.e. inside the float64 band) plus a margin of 2^10 ulp of the largest partial
    sum of its field (the device adds the bias first and may round differently by an ulp or so), or at class B / C distance.
    J must be dyadic (J s exact).  Returns (b, cls (n,) by position, first-sweep state)."""
    rng = np.random.default_rng(0) if rng is None else rng
    J = np.asarray(J, dtype=np.float64)
    n = J.shape[0]
    s = np.asarray(state).astype(np.int8).copy()
    sf = s.astype(np.float64)
    rowabs = np.abs(J).sum(axis=1)
    b = np.zeros(n)
    cls = np.full(n, "R", dtype="<U1")
    idx = range(n) if order is None else [int(v) for v in order]
    picks = rng.integers(0, 1 << 30, size=n)
    outs = rng.integers(0, 2, size=n)
    for k, i in enumerate(idx):
        u = dense_uniform(i, sweep0, seed, replica)
        ci = float(J[i] @ sf)  # exact: J is dyadic
        lg = logit(u)
        o = int(outs[k])
        sgn = 1.0 if o else -1.0
        bound = abs(ci) + rowabs[i] + 40.0 * T  # largest |partial sum| of the field, bias included (|x| <= 40)
        margin = 2.0 ** 10 * 2.0 ** -52 * bound / T
        xt, cl = None, "R"
        if abs(lg) <= 12.0:
            first = int(picks[k]) % len(classes)
            for j in range(len(classes)):
                cl = classes[(first + j) % len(classes)]
                if cl == "A":
                    kmax = min(1024, int((0.4 * BAND_EXACT * (1.0 + abs(lg)) - margin) * u * (1.0 - u) / U53))
                    if kmax >= 64:
                        xt = lg + sgn * (int(rng.integers(64, kmax + 1)) * U53 / (u * (1.0 - u)) + margin)
                elif cl in "BC":
                    xt = lg + sgn * (3e-9 if cl == "B" else 2e-4) * (1.0 + abs(lg))
                if xt is not None:
                    break
        if xt is None:
            xt, cl = float(rng.normal()) * 3.0, "R"
        b[i] = xt * T - ci
        h = ci + b[i]
        new = 1 if u < _sig(h / T) else 0
        if cl != "R":
            assert new == o and (h / T > lg) == bool(o), (i, cl)
        cls[k] = cl
        s[i] = sf[i] = new
    return b, cls, s

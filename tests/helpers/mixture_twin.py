"""CPU float32 twin of K3's Gaussian-mixture kernels (csrc/langevin.hip k3_mixture_lane / k3_mixture_wg).

The noise is the separable kernel's stream, taken from the oracle (oracle.langevin_normals_f32: quad q of chain c at step s).  The
gradient sum_i c_i (x - mu_i), c_i = exp(a_i - m) / (sigma_i^2 Z), is formed in float64 from the float32 state and the float32
parameters the device holds (log w, 1/sigma^2, log eps, each rounded once from float64 on the host), and rounded to float32 once;
the update is the kernel's x <- fma(scale, xi, fma(-g, dt/gamma, x)) in float32.  The device evaluates the same expression in
float32 in its own order: the tests compare with a tolerance."""
import numpy as np

from oracle import oracle as ora


def device_params(centers, weights, sigma=1.0, eps=1e-10):
    """The float32 parameters set_mixture hands the device."""
    c = np.asarray(centers, dtype=np.float64)
    K = c.shape[0]
    w = np.broadcast_to(np.asarray(weights, dtype=np.float64), (K,))
    sg = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (K,))
    lw = np.log(w).astype(np.float32)
    iv = (1.0 / sg ** 2).astype(np.float32)
    leps = np.float32(np.log(eps)) if eps > 0 else np.float32(-np.inf)
    return c.astype(np.float32), lw, iv, leps


def gradient_f32(x, c32, lw, iv, leps):
    """x: (n, d) float32 -> (n, d) float32 (float64 arithmetic, one rounding)."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    c64, lw64, iv64 = c32.astype(np.float64), lw.astype(np.float64), iv.astype(np.float64)
    diff = x64[:, None, :] - c64[None, :, :]                     # (n, K, d)
    a = lw64[None, :] - 0.5 * iv64[None, :] * np.sum(diff ** 2, axis=2)
    m = np.max(a, axis=1, keepdims=True)
    r = np.exp(a - m)
    with np.errstate(over="ignore"):  # (far out on the eps plateau exp(log eps - m) is +inf, as on the device: c = 0)
        z = np.sum(r, axis=1, keepdims=True) + np.exp(np.float64(leps) - m)
    cc = r * iv64[None, :] / z
    return np.einsum("nk,nkd->nd", cc, diff).astype(np.float32)


def _fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def normals(n_chains, dim, step, seed, chain0=0):
    quads = (dim + 3) // 4
    out = np.empty((n_chains, 4 * quads), np.float32)
    for c in range(n_chains):
        for q in range(quads):
            out[c, 4 * q:4 * q + 4] = ora.langevin_normals_f32(q, chain0 + c, step, seed)
    return out[:, :dim]


def step_coefficients(dt, gamma, T):
    """a = dt / gamma and scale = sqrt(2 T dt / gamma) as the kernel's host code forms them (float32)."""
    dt32, g32, T32 = np.float32(dt), np.float32(gamma), np.float32(T)
    a = np.float32(dt32 / g32)
    scale = np.float32(np.sqrt(np.float32(np.float32(np.float32(2.0) * T32) * dt32) / g32))
    return a, scale


def mixture_f32(x, centers, weights, sigma, eps, n_steps, dt, gamma, T, seed, step0=0, chain0=0, trajectory=False):
    """x: (n_chains, dim) float32 -> x_final or (x_final, traj (n_steps, n_chains, dim))."""
    xx = np.array(x, dtype=np.float32, copy=True)
    if xx.ndim == 1:
        xx = xx[None, :]
    n, d = xx.shape
    c32, lw, iv, leps = device_params(centers, weights, sigma, eps)
    a, scale = step_coefficients(dt, gamma, T)
    traj = np.zeros((n_steps, n, d), np.float32) if trajectory else None
    for s in range(n_steps):
        g = gradient_f32(xx, c32, lw, iv, leps)
        xi = normals(n, d, step0 + s, seed, chain0)
        xx = _fma32(scale, xi, _fma32(-g, a, xx))
        if trajectory:
            traj[s] = xx
    return (xx, traj) if trajectory else xx

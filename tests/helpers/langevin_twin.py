"""CPU float64 twin of K3's noise stream and separable step (csrc/langevin.hip, the stream contract in its header), NumPy only.

Philox4x32-10 over arrays of counters, counter layout of oracle/tsu_oracle.c ora_langevin_normals_f32: ctr = (q, chain, step, tag),
key = (seed low, seed high).  Box-Muller in float64 from the 24-bit uniforms the contract names: u1 = ((w >> 8) + 1) / 2^24,
u2 = (w >> 8) / 2^24, r = sqrt(-2 ln u1), angle = 2 pi u2.  The oracle restates this in float32 with libm, the device with its
native log2 / sqrt / sin / cos units: this twin is the yardstick both are measured against.  Chain and step counters wrap as uint32,
as `chain0 + ch` and `step0 + s` do in the kernels."""
import numpy as np

TAG_LANGEVIN = 3
TAG_LANGEVIN_RESTART = 5

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr: (..., 4) uint32, key: (2,) uint32 -> (..., 4) uint32."""
    c = np.asarray(ctr, dtype=np.uint32).astype(np.uint64)
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2  # (32 x 32 bits: no overflow in uint64)
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _LO
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _u32(v):
    """Integers of any size (Python ints, int64 or uint64 arrays) reduced modulo 2^32."""
    a = np.asarray(v)
    if a.dtype == object:
        a = np.array([int(t) & 0xFFFFFFFF for t in a.ravel()], dtype=np.uint64).reshape(a.shape)
    return (a.astype(np.uint64) & _LO).astype(np.uint32)


def wrap_ids(first, n):
    """first, first + 1, ..., first + n - 1 as uint32 counters (mod 2^32)."""
    return ((np.uint64(int(first) & 0xFFFFFFFF) + np.arange(n, dtype=np.uint64)) & _LO).astype(np.uint32)


def words(q, chain, step, tag, seed):
    """The four Philox words of quad q of `chain` at `step` (arguments broadcast against each other) -> (..., 4) uint32."""
    q, chain, step, tag = np.broadcast_arrays(_u32(q), _u32(chain), _u32(step), _u32(tag))
    seed = int(seed)
    return philox4x32_10(np.stack([q, chain, step, tag], axis=-1), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def normals_f64(q, chain, step, tag, seed):
    """-> (xi (..., 4), r (..., 2), angle (..., 2)), all float64: xi[2p] = r[p] cos(angle[p]), xi[2p + 1] = r[p] sin(angle[p])."""
    w = words(q, chain, step, tag, seed)
    m = (w >> np.uint32(8)).astype(np.float64)
    u1 = (m[..., 0::2] + 1.0) / 16777216.0
    u2 = m[..., 1::2] / 16777216.0
    r = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * np.pi * u2
    xi = np.empty(w.shape, np.float64)
    xi[..., 0::2] = r * np.cos(ang)
    xi[..., 1::2] = r * np.sin(ang)
    return xi, r, ang


def chain_normals_f64(n_chains, dim, step, seed, chain0=0, tag=TAG_LANGEVIN):
    """(n_chains, dim) float64: element i of chain c takes normal i & 3 of quad i >> 2, chain id chain0 + c (mod 2^32)."""
    quads = (dim + 3) // 4
    xi, _, _ = normals_f64(np.arange(quads, dtype=np.uint32)[None, :], wrap_ids(chain0, n_chains)[:, None], step, tag, seed)
    return xi.reshape(n_chains, 4 * quads)[:, :dim]


def restart_f64(x_init, amp, n_chains, seed, chain0=0):
    """x_init + amp N(0, 1) with the restart tag at step 0 (k3_restart) -> (n_chains, dim) float64; amp as the device's float32."""
    xi0 = np.asarray(x_init, dtype=np.float32).astype(np.float64).ravel()
    return xi0[None, :] + float(np.float32(amp)) * chain_normals_f64(n_chains, xi0.size, 0, seed, chain0, TAG_LANGEVIN_RESTART)


def quadratic_f64(x, k, mu, n_steps, dt, gamma, T, seed, step0=0, chain0=0, trajectory=False):
    """n_steps of x <- x + (-k (x - mu)) dt / gamma + sqrt(2 T dt / gamma) xi in float64; k, mu, dt, gamma, T as the float32 values
    the device holds, x as given (a float32 state converts exactly; a float64 one continues a twin's run).
    x: (n_chains, dim).  Returns x_final or (x_final, traj (n_steps, n_chains, dim))."""
    xx = np.array(x, dtype=np.float64)
    if xx.ndim == 1:
        xx = xx[None, :]
    n, d = xx.shape
    kk = np.broadcast_to(np.asarray(k, dtype=np.float32).astype(np.float64), (d,))
    mm = np.broadcast_to(np.asarray(mu, dtype=np.float32).astype(np.float64), (d,))
    dt, gamma, T = (float(np.float32(v)) for v in (dt, gamma, T))
    a, scale = dt / gamma, np.sqrt(2.0 * T * dt / gamma)
    traj = np.zeros((n_steps, n, d)) if trajectory else None
    for s, st in enumerate(wrap_ids(step0, n_steps)):
        xx = xx + (-(kk * (xx - mm))) * a + scale * chain_normals_f64(n, d, st, seed, chain0)
        if trajectory:
            traj[s] = xx
    return (xx, traj) if trajectory else xx

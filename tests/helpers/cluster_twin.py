"""NumPy twin of K6's Swendsen-Wang step (csrc/ising2d_cluster.hip), bit for bit.

Step t of a (rows, cols) lattice of +-1 spins with key = seed:
  bond  site (r, c): W = Philox4x32-10(c >> 1, r, t, TAG_SW_BOND | replica << 8); right bond (to c + 1, wrapping on a periodic
        lattice) active iff J s s' > 0 and W[2 (c & 1)] < thr, down bond likewise with W[2 (c & 1) + 1];
        thr = floor(p 2^32), p = -expm1(-2|J|/T) in float64
  label connected components of the active bonds (scipy.sparse.csgraph), root = smallest index r * cols + c of the component
  flip  the cluster rooted at (r, c) flips iff bit 31 of word c & 3 of Philox(c >> 2, r, t, TAG_SW_FLIP | replica << 8) is set
"""
import math

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

TAG_SW_BOND = 6
TAG_SW_FLIP = 7
_MASK = np.uint64(0xFFFFFFFF)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10: counters broadcast against each other, scalar key; four uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) & _MASK for x in (c0, c1, c2, c3)])
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = _M0 * c0
        p1 = _M1 * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c1 = p1 & _MASK
        c3 = p0 & _MASK
        c0, c2 = n0, n2
        k0 = (k0 + _W0) & 0xFFFFFFFF
        k1 = (k1 + _W1) & 0xFFFFFFFF
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def threshold(J, T):
    if not T > 0:
        raise ValueError("Temperature must be positive")
    p = -math.expm1(-2.0 * abs(float(J)) / float(T))
    return int(math.floor(p * 4294967296.0))


def _words(seed, r, c, t, tag):
    return philox4x32_10(c, r, t, tag, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def labels(spins, periodic, J, T, seed, t, replica=0):
    """(root index per site (rows, cols) int64, active right bonds, active down bonds)."""
    s = np.asarray(spins, dtype=np.int64)
    rows, cols = s.shape
    n = rows * cols
    thr = threshold(J, T)
    R, Cc = np.meshgrid(np.arange(rows, dtype=np.int64), np.arange(cols, dtype=np.int64), indexing="ij")
    w = _words(int(seed), R, Cc >> 1, int(t), TAG_SW_BOND | (int(replica) << 8))
    odd = (Cc & 1) == 1
    u_right = np.where(odd, w[2], w[0]).astype(np.uint64)
    u_down = np.where(odd, w[3], w[1]).astype(np.uint64)
    jsign = int(np.sign(J))
    idx = np.arange(n, dtype=np.int64).reshape(rows, cols)
    right = np.roll(idx, -1, axis=1)
    down = np.roll(idx, -1, axis=0)
    ok_r = np.ones((rows, cols), bool) if periodic else (Cc < cols - 1)
    ok_d = np.ones((rows, cols), bool) if periodic else (R < rows - 1)
    s_r, s_d = np.roll(s, -1, axis=1), np.roll(s, -1, axis=0)
    act_r = ok_r & (jsign * s * s_r > 0) & (u_right < np.uint64(thr))
    act_d = ok_d & (jsign * s * s_d > 0) & (u_down < np.uint64(thr))
    src = np.concatenate([idx[act_r], idx[act_d]])
    dst = np.concatenate([right[act_r], down[act_d]])
    g = coo_matrix((np.ones(src.size, np.int8), (src, dst)), shape=(n, n))
    ncomp, lab = connected_components(g, directed=False)
    root = np.full(ncomp, n, dtype=np.int64)
    np.minimum.at(root, lab, np.arange(n, dtype=np.int64))
    return root[lab].reshape(rows, cols), act_r, act_d


def step(spins, periodic, J, T, seed, t, replica=0):
    """One Swendsen-Wang step; returns a new int8 array."""
    s = np.asarray(spins, dtype=np.int8)
    rows, cols = s.shape
    roots, _, _ = labels(s, periodic, J, T, seed, t, replica)
    u = np.unique(roots)
    rr, rc = u // cols, u % cols
    w = _words(int(seed), rr, rc >> 2, int(t), TAG_SW_FLIP | (int(replica) << 8))
    word = np.choose((rc & 3).astype(np.int64), w)
    flip_root = (word >> np.uint32(31)) == 1
    flip = flip_root[np.searchsorted(u, roots)]
    return np.where(flip, -s, s).astype(np.int8)


def sweep(spins, periodic, J, T, n_steps, seed, step0=0, replica=0):
    """n_steps steps with counters step0 .. step0 + n_steps - 1."""
    s = np.asarray(spins, dtype=np.int8)
    for k in range(int(n_steps)):
        s = step(s, periodic, J, T, seed, int(step0) + k, replica)
    return s


def bond_sum(spins, periodic):
    """sum over nearest-neighbour bonds of s_i s_j (energy = -J * this)."""
    s = np.asarray(spins, dtype=np.int64)
    if periodic:
        return int(np.sum(s * np.roll(s, -1, 1)) + np.sum(s * np.roll(s, -1, 0)))
    return int(np.sum(s[:, :-1] * s[:, 1:]) + np.sum(s[:-1, :] * s[1:, :]))

"""NumPy twin of K8's Swendsen-Wang step on a 3-D lattice with per-bond couplings (csrc/ising3d_cluster.hip), bit for bit.

Step t of a (D, R, C) lattice of +-1 spins and float32 couplings J_right, J_down, J_layer, key = seed, periodic = (p_z, p_r, p_c)
(a bool means all three); global row rho = z R + r, site index i = rho C + c:
  bond  b = (i, j) with stored coupling J_b is active iff J_b s_i s_j > 0 and u_b < thr_b; thr_b = floor(p_b 2^32),
        p_b = -expm1(-2 |J_b| / T) in float64 from the fp32 value widened; J_b = 0 is never active; an open axis has no bond
        from its last slice
  u_b   right and down bonds of (z, r, c): W = Philox4x32-10(c >> 1, rho, t, TAG_SW_BOND | replica << 8), right W[2 (c & 1)], down
        W[2 (c & 1) + 1]; layer bond to (z + 1, r, c) (wrapping on a periodic z axis): word c & 3 of
        Philox(c >> 2, rho, t, TAG_SW_LAYER | replica << 8)
  label connected components of the active bonds (scipy.sparse.csgraph), root = smallest site index of the component
  flip  the cluster rooted at (rho, c) flips iff bit 31 of word c & 3 of Philox(c >> 2, rho, t, TAG_SW_FLIP | replica << 8) is set
With D = 1, open z and constant J this is cluster_twin.step on (R, C).
"""
import importlib.util
import os

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

_spec = importlib.util.spec_from_file_location("cluster_twin", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                           "cluster_twin.py"))
_ct = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_ct)
philox4x32_10 = _ct.philox4x32_10
TAG_SW_BOND = _ct.TAG_SW_BOND
TAG_SW_FLIP = _ct.TAG_SW_FLIP
TAG_SW_LAYER = 10


def axes(periodic):
    """(p_z, p_r, p_c) from a bool or a triple."""
    if isinstance(periodic, (bool, np.bool_)):
        return (bool(periodic),) * 3
    p = tuple(bool(x) for x in periodic)
    assert len(p) == 3
    return p


def thresholds(J, T):
    """uint64 thr_b of every bond: floor(-expm1(-2 |J| / T) 2^32) in float64 from the fp32 couplings (may be 2^32)."""
    if not T > 0:
        raise ValueError("Temperature must be positive")
    j64 = np.abs(np.asarray(J, dtype=np.float32).astype(np.float64))
    p = -np.expm1((-2.0 * j64) / float(T))
    return np.floor(p * 4294967296.0).astype(np.uint64)


def _words(seed, rho, c, t, tag):
    return philox4x32_10(c, rho, t, tag, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)


def bond_uniforms(shape, seed, t, replica=0):
    """(u_right, u_down, u_layer): (D, R, C) uint64 arrays of the bonds' 32-bit uniforms."""
    D, R, C = shape
    rho = np.arange(D * R, dtype=np.int64).reshape(D, R, 1)
    c = np.arange(C, dtype=np.int64).reshape(1, 1, C)
    rho, c = np.broadcast_arrays(rho, c)
    w = _words(seed, rho, c >> 1, int(t), TAG_SW_BOND | (int(replica) << 8))
    odd = (c & 1) == 1
    u_right = np.where(odd, w[2], w[0]).astype(np.uint64)
    u_down = np.where(odd, w[3], w[1]).astype(np.uint64)
    wl = _words(seed, rho, c >> 2, int(t), TAG_SW_LAYER | (int(replica) << 8))
    u_layer = np.choose(c & 3, wl).astype(np.uint64)
    return u_right, u_down, u_layer


def active_bonds(spins, periodic, J_right, J_down, J_layer, T, seed, t, replica=0):
    """(act_right, act_down, act_layer): bool (D, R, C) arrays, the bond from each site along +c, +r, +z."""
    s = np.asarray(spins, dtype=np.int64)
    assert s.ndim == 3
    shape = s.shape
    per = axes(periodic)
    us = bond_uniforms(shape, seed, t, replica)
    idx = np.indices(shape)
    out = []
    for axis, J, u in ((2, J_right, us[0]), (1, J_down, us[1]), (0, J_layer, us[2])):
        j32 = np.asarray(J, dtype=np.float32).reshape(shape)
        has = np.ones(shape, bool) if per[axis] else idx[axis] < shape[axis] - 1
        sat = np.sign(j32).astype(np.int64) * s * np.roll(s, -1, axis=axis) > 0
        out.append(has & sat & (u < thresholds(j32, T)))
    return tuple(out)


def labels(spins, periodic, J_right, J_down, J_layer, T, seed, t, replica=0):
    """(root index per site (D, R, C) int64, (act_right, act_down, act_layer))."""
    s = np.asarray(spins)
    shape = s.shape
    n = s.size
    act = active_bonds(s, periodic, J_right, J_down, J_layer, T, seed, t, replica)
    idx = np.arange(n, dtype=np.int64).reshape(shape)
    src = np.concatenate([idx[a] for a in act])
    dst = np.concatenate([np.roll(idx, -1, axis=axis)[a] for axis, a in zip((2, 1, 0), act)])
    g = coo_matrix((np.ones(src.size, np.int8), (src, dst)), shape=(n, n))
    ncomp, lab = connected_components(g, directed=False)
    root = np.full(ncomp, n, dtype=np.int64)
    np.minimum.at(root, lab, np.arange(n, dtype=np.int64))
    return root[lab].reshape(shape), act


def flip_of_roots(roots, cols, seed, t, replica=0):
    """bool per entry of `roots` (site indices): the coin of the cluster rooted there."""
    u = np.asarray(roots, dtype=np.int64)
    rho, rc = u // cols, u % cols
    w = _words(seed, rho, rc >> 2, int(t), TAG_SW_FLIP | (int(replica) << 8))
    word = np.choose(rc & 3, w)
    return (word >> np.uint32(31)) == 1


def step(spins, periodic, J_right, J_down, J_layer, T, seed, t, replica=0):
    """One Swendsen-Wang step; returns a new int8 array."""
    s = np.asarray(spins, dtype=np.int8)
    roots, _ = labels(s, periodic, J_right, J_down, J_layer, T, seed, t, replica)
    u = np.unique(roots)
    flip = flip_of_roots(u, s.shape[2], seed, t, replica)[np.searchsorted(u, roots)]
    return np.where(flip, -s, s).astype(np.int8)


def sweep(spins, periodic, J_right, J_down, J_layer, T, n_steps, seed, step0=0, replica=0):
    """n_steps steps with counters step0 .. step0 + n_steps - 1."""
    s = np.asarray(spins, dtype=np.int8)
    for k in range(int(n_steps)):
        s = step(s, periodic, J_right, J_down, J_layer, T, seed, int(step0) + k, replica)
    return s

"""NumPy twin of K8's ghost-spin Swendsen-Wang step (csrc/ising3d_cluster.hip, tsu_ising3d_cluster_sweep_field), bit for bit.

The step of cluster3d_twin (the same bonds, words, tags and coins) plus, for step t of a (D, R, C) lattice with float32 field h,
key = seed, global row rho = z R + r, site index i = rho C + c:
  ghost   the ghost bond of site i is active iff h_i s_i > 0 and u_g < thr(|h_i|), thr = cluster3d_twin.thresholds (may be 2^32);
          h_i = 0 is never active; u_g = word c & 3 of Philox4x32-10(c >> 2, rho, t, TAG_SW_GHOST | replica << 8)
  frozen  a component of the active bonds that contains an active ghost bond keeps its spins and draws no coin; every other
          component flips by the coin of its smallest site index (cluster3d_twin.flip_of_roots)
The ghost is node n = D R C of the graph handed to scipy's connected_components; a component is frozen iff it is node n's.
With h = None or all zeros this is cluster3d_twin.step.  The step samples exp(-E / T) / Z for E = lattice3d_twin.energy.
"""
import importlib.util
import os

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

_spec = importlib.util.spec_from_file_location("cluster3d_twin", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                             "cluster3d_twin.py"))
_c3 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_c3)
philox4x32_10 = _c3.philox4x32_10
active_bonds = _c3.active_bonds
thresholds = _c3.thresholds
flip_of_roots = _c3.flip_of_roots
axes = _c3.axes
TAG_SW_GHOST = 12


def ghost_uniforms(shape, seed, t, replica=0):
    """(D, R, C) uint64: every site's u_g."""
    D, R, C = shape
    rho = np.arange(D * R, dtype=np.int64).reshape(D, R, 1)
    c = np.arange(C, dtype=np.int64).reshape(1, 1, C)
    rho, c = np.broadcast_arrays(rho, c)
    w = philox4x32_10(c >> 2, rho, int(t), TAG_SW_GHOST | (int(replica) << 8), int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    return np.choose(c & 3, w).astype(np.uint64)


def active_ghost(spins, h, T, seed, t, replica=0):
    """bool (D, R, C): the sites whose ghost bond is active (h=None: none)."""
    s = np.asarray(spins, dtype=np.int64)
    if h is None:
        return np.zeros(s.shape, bool)
    h32 = np.asarray(h, dtype=np.float32).reshape(s.shape)
    sat = np.sign(h32).astype(np.int64) * s > 0
    return sat & (ghost_uniforms(s.shape, seed, t, replica) < thresholds(h32, T))


def labels(spins, periodic, J_right, J_down, J_layer, h, T, seed, t, replica=0):
    """(root (D, R, C) int64: the smallest site index of the site's component of the lattice bonds and ghost bonds together,
    frozen (D, R, C) bool: the component holds an active ghost bond, (act_right, act_down, act_layer), act_ghost)."""
    s = np.asarray(spins)
    shape, n = s.shape, s.size
    act = active_bonds(s, periodic, J_right, J_down, J_layer, T, seed, t, replica)
    ghost = active_ghost(s, h, T, seed, t, replica)
    idx = np.arange(n, dtype=np.int64).reshape(shape)
    src = np.concatenate([idx[a] for a in act] + [idx[ghost]])
    dst = np.concatenate([np.roll(idx, -1, axis=axis)[a] for axis, a in zip((2, 1, 0), act)] + [np.full(int(ghost.sum()), n, np.int64)])
    g = coo_matrix((np.ones(src.size, np.int8), (src, dst)), shape=(n + 1, n + 1))
    ncomp, lab = connected_components(g, directed=False)
    root = np.full(ncomp, n, dtype=np.int64)
    np.minimum.at(root, lab[:n], np.arange(n, dtype=np.int64))
    frozen = lab[:n] == lab[n]
    return root[lab[:n]].reshape(shape), frozen.reshape(shape), act, ghost


def step(spins, periodic, J_right, J_down, J_layer, h, T, seed, t, replica=0):
    """One ghost-spin Swendsen-Wang step; returns a new int8 array."""
    s = np.asarray(spins, dtype=np.int8)
    roots, frozen, _, _ = labels(s, periodic, J_right, J_down, J_layer, h, T, seed, t, replica)
    u = np.unique(roots)
    flip = flip_of_roots(u, s.shape[2], seed, t, replica)[np.searchsorted(u, roots)] & ~frozen
    return np.where(flip, -s, s).astype(np.int8)


def sweep(spins, periodic, J_right, J_down, J_layer, h, T, n_steps, seed, step0=0, replica=0):
    """n_steps steps with counters step0 .. step0 + n_steps - 1."""
    s = np.asarray(spins, dtype=np.int8)
    for k in range(int(n_steps)):
        s = step(s, periodic, J_right, J_down, J_layer, h, T, seed, int(step0) + k, replica)
    return s

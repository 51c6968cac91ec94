"""NumPy twin of K12, the q-state Potts lattice with per-bond couplings and per-site colour fields (csrc/potts_disorder.hip,
csrc/potts_disorder_dev.h), bit for bit.

State: (D, R, C) int8 colours 0 .. q - 1, or (R, C), which is the lattice (1, R, C) with an open z axis; periodic = one flag per axis
(a bool means every axis of the shape).  E = -sum_bonds J_b [s_i = s_j] - sum_i h[i][s_i].  Disorder as the device stores it: fp32
arrays of the lattice's shape, the entry at a site the bond that leaves it in +c (J_right), +r (J_down), +z (J_layer, absent in 2-D);
h of shape (q,) + shape, colour-major, or None.  Global row rho = z R + r, site index i = rho C + c.

Heat bath, half-sweep hs = 2 sweep + colour (32-bit words), colour = (z + r + c) & 1, key = seed:
  u     K10's site uniform (potts3d_twin.site_uniforms)
  a_c   = float64(h[c][i]) (0.0 without a field), then + float64(J_k) for every existing neighbour k in the order z-1, z+1, r-1,
          r+1, c-1, c+1 that shows colour c
  w_c   = exp((a_c - max a) / T): math.exp, the C library's exp that the host build of the rule uses
  Z_c   = Z_{c-1} + w_c in colour order; thr_c = floor(Z_c / Z_{q-1} 2^32 + 0.5) for c < q - 1, thr_{q-1} = 2^32
  new colour: the smallest c with u < thr_c
Swendsen-Wang step t (every coupling >= 0, no field): K10's words (potts3d_twin.bond_uniforms); a bond is active iff it exists, its two
colours agree and u < floor(-expm1(-J_b / T) 2^32) (math.expm1); the label is the smallest site index, the root's colour (W q) >> 32.

A decision is `fragile` when u lies within one unit of the real-valued threshold it is compared with: only such a decision can depend
on whose exp or expm1 ran.  `sweep`, `cluster_sweep` and the chains count them; the GPU tests run inputs that have none.
"""
import importlib.util
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


p3 = _load("potts3d_twin")
philox4x32_10, state_code = p3.philox4x32_10, p3.state_code
TWO32 = 4294967296.0
MAX_Q = 8
SMALL_SITES = 16384
_exp = np.vectorize(math.exp, otypes=[np.float64])
_expm1 = np.vectorize(math.expm1, otypes=[np.float64])


def lattice(shape, periodic):
    """(shape3, (p_z, p_r, p_c)) of a 2-D or 3-D shape."""
    shape = tuple(int(n) for n in shape)
    if len(shape) == 2:
        p = (bool(periodic),) * 2 if isinstance(periodic, (bool, np.bool_)) else tuple(bool(x) for x in periodic)
        assert len(p) == 2
        return (1,) + shape, (False,) + p
    assert len(shape) == 3
    return shape, p3.axes(periodic)


def as_disorder(shape, periodic, J, h=None, q=None):
    """The fp32 arrays the device stores, as 3-D arrays: (jr, jd, jl, h or None).  J = (J_right, J_down[, J_layer]) of the lattice's
    own shape; on an open axis the last slice must be 0 (asserted, as the library refuses it)."""
    shape3, per = lattice(shape, periodic)
    arrs = [np.asarray(a, dtype=np.float32).reshape(shape3) for a in J]
    if len(arrs) == 2:
        arrs.append(np.zeros(shape3, np.float32))
    jr, jd, jl = arrs
    assert per[2] or not jr[:, :, -1].any()
    assert per[1] or not jd[:, -1, :].any()
    assert per[0] or not jl[-1, :, :].any()
    hh = None if h is None else np.asarray(h, dtype=np.float32).reshape((-1,) + shape3)
    assert hh is None or q is None or hh.shape[0] == q
    return jr, jd, jl, hh


def random_disorder(shape, periodic, q, rng, kind="gaussian", field=True):
    """(J, h) of the lattice's own shape: Gaussian couplings of both signs or couplings from {0, 1, 2}, the last slice of an open
    axis zeroed; h Gaussian, (q,) + shape, or None."""
    shape = tuple(shape)
    _, per = lattice(shape, periodic)
    per = per[3 - len(shape):]
    J = []
    for k in range(len(shape)):
        a = rng.normal(size=shape) if kind == "gaussian" else rng.integers(0, 3, size=shape).astype(np.float64)
        axis = len(shape) - 1 - k
        if not per[axis]:
            a[(slice(None),) * axis + (-1,)] = 0.0
        J.append(a.astype(np.float32))
    h = rng.normal(size=(q,) + shape).astype(np.float32) if field else None
    return tuple(J), h


def constant_couplings(shape, periodic, J):
    """Every existing bond J: arrays of the lattice's own shape, the last slice of an open axis 0."""
    shape = tuple(shape)
    _, per = lattice(shape, periodic)
    per = per[3 - len(shape):]
    out = []
    for k in range(len(shape)):
        a = np.full(shape, J, np.float32)
        axis = len(shape) - 1 - k
        if not per[axis]:
            a[(slice(None),) * axis + (-1,)] = 0.0
        out.append(a)
    return tuple(out)


def _neighbours(s, per, jr, jd, jl):
    """The six (colour, coupling) arrays in the contract's order; colour -1 where an open axis has no neighbour."""
    s = np.asarray(s, dtype=np.int64)
    out = []
    for axis, J in ((0, jl), (1, jd), (2, jr)):
        for shift in (1, -1):
            nb = np.roll(s, shift, axis).copy()
            if not per[axis]:
                edge = [slice(None)] * 3
                edge[axis] = 0 if shift == 1 else -1
                nb[tuple(edge)] = -1
            # the bond to the neighbour before a site is stored at that neighbour, the bond to the one after it at the site
            out.append((nb, (np.roll(J, 1, axis) if shift == 1 else J).astype(np.float64)))
    return out


def site_sums(s, q, per, jr, jd, jl, h):
    """Step 1: a[c] of every site, (q, D, R, C) float64."""
    nbs = _neighbours(s, per, jr, jd, jl)
    a = np.zeros((q,) + np.shape(s), np.float64) if h is None else h.astype(np.float64)
    a = a.copy()
    for c in range(q):
        for nb, J in nbs:
            a[c] = np.where(nb == c, a[c] + J, a[c])
    return a


def thresholds(a, T):
    """Steps 2 - 5 for sums a of shape (q, ...): (thr as uint64 with thr[q - 1] = 2^32, the real-valued Z_c / Z_{q-1} 2^32)."""
    q = a.shape[0]
    w = _exp((a - a.max(axis=0)) / float(T))
    Z = np.empty_like(w)
    Z[0] = w[0]
    for c in range(1, q):
        Z[c] = Z[c - 1] + w[c]
    real = Z / Z[q - 1] * TWO32
    thr = np.floor(real + 0.5).astype(np.uint64)
    thr[q - 1] = np.uint64(2 ** 32)
    return thr, real


def pick(thr, u):
    u = np.asarray(u).astype(np.uint64)
    colour = np.full(u.shape, thr.shape[0] - 1, np.int8)
    for c in range(thr.shape[0] - 2, -1, -1):
        colour = np.where(u < thr[c], np.int8(c), colour)
    return colour


def site_thresholds(a, T):
    """One site: thr[0 .. q - 1] as Python ints (tsu_potts_dis_site_thresholds)."""
    return [int(v) for v in thresholds(np.asarray(a, dtype=np.float64).reshape(-1, 1), T)[0][:, 0]]


def sweep(spins, q, periodic, J, h, T, n_sweeps, seed, sweep0=0, replica=0, with_fragile=False):
    """n_sweeps heat-bath sweeps; returns a new int8 array of the input's shape (with_fragile: and the number of fragile decisions)."""
    s0 = np.array(spins, dtype=np.int8)
    shape3, per = lattice(s0.shape, periodic)
    jr, jd, jl, hh = as_disorder(s0.shape, periodic, J, h, q)
    s = s0.reshape(shape3)
    colour_of = p3.colours(shape3)
    n_fragile = 0
    for k in range(int(n_sweeps)):
        sw = (int(sweep0) + k) & 0xFFFFFFFF
        for colour in (0, 1):
            hs = (2 * sw + colour) & 0xFFFFFFFF
            u = p3.site_uniforms(shape3, hs, seed, replica)
            thr, real = thresholds(site_sums(s, q, per, jr, jd, jl, hh), T)
            mine = colour_of == colour
            n_fragile += int(np.count_nonzero((np.abs(u.astype(np.float64)[None] - real[:q - 1]) <= 1.0) & mine[None]))
            s = np.where(mine, pick(thr, u), s).astype(np.int8)
    s = s.reshape(s0.shape)
    return (s, n_fragile) if with_fragile else s


def fragile(spins, q, periodic, J, h, T, n_sweeps, seed, sweep0=0, replica=0):
    """The fragile decisions of `sweep` on these inputs."""
    return sweep(spins, q, periodic, J, h, T, n_sweeps, seed, sweep0, replica, with_fragile=True)[1]


# ---------------------------------------------------------------- Swendsen-Wang steps
def bond_thresholds(J, T):
    """floor(-expm1(-J / T) 2^32) of every stored bond, and the real-valued product."""
    real = -_expm1(-np.asarray(J, dtype=np.float64) / float(T)) * TWO32
    return np.floor(real).astype(np.uint64), real


def cluster_step(spins, q, periodic, J, T, seed, t, replica=0, with_fragile=False):
    """One Swendsen-Wang step on non-negative couplings; returns a new int8 array."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    s0 = np.asarray(spins, dtype=np.int8)
    shape3, per = lattice(s0.shape, periodic)
    jr, jd, jl, _ = as_disorder(s0.shape, periodic, J)
    assert min(jr.min(), jd.min(), jl.min()) >= 0
    s = s0.reshape(shape3).astype(np.int64)
    n, cols = s.size, shape3[2]
    us = p3.bond_uniforms(shape3, seed, t, replica)
    where = np.indices(shape3)
    idx = np.arange(n, dtype=np.int64).reshape(shape3)
    src, dst, n_fragile = [], [], 0
    for axis, u, Jb in ((2, us[0], jr), (1, us[1], jd), (0, us[2], jl)):
        has = np.ones(shape3, bool) if per[axis] else where[axis] < shape3[axis] - 1
        thr, real = bond_thresholds(Jb, T)
        sat = has & (s == np.roll(s, -1, axis))
        n_fragile += int(np.count_nonzero(sat & (np.abs(u.astype(np.float64) - real) <= 1.0)))
        act = sat & (u < thr)
        src.append(idx[act])
        dst.append(np.roll(idx, -1, axis)[act])
    src, dst = np.concatenate(src), np.concatenate(dst)
    ncomp, lab = connected_components(coo_matrix((np.ones(src.size, np.int8), (src, dst)), shape=(n, n)), directed=False)
    root = np.full(ncomp, n, dtype=np.int64)
    np.minimum.at(root, lab, np.arange(n, dtype=np.int64))
    roots = root[lab]
    uq = np.unique(roots)
    rho, rc = uq // cols, uq % cols
    w = p3._words(seed, rho, rc >> 2, int(t), p3.TAG_SW_FLIP | (int(replica) << 8))
    word = np.choose((rc & 3).astype(np.int64), w).astype(np.uint64)
    colour = ((word * np.uint64(q)) >> np.uint64(32)).astype(np.int8)
    out = colour[np.searchsorted(uq, roots)].astype(np.int8).reshape(s0.shape)
    return (out, n_fragile) if with_fragile else out


def cluster_sweep(spins, q, periodic, J, T, n_steps, seed, step0=0, replica=0, with_fragile=False):
    s = np.asarray(spins, dtype=np.int8)
    n_fragile = 0
    for k in range(int(n_steps)):
        s, f = cluster_step(s, q, periodic, J, T, seed, int(step0) + k, replica, with_fragile=True)
        n_fragile += f
    return (s, n_fragile) if with_fragile else s


# ---------------------------------------------------------------- observables
def measure(spins, q, periodic):
    """(n_eq, N_0 .. N_{q-1}): exact integers, as K10 counts them (a periodic axis of length 2 counts its double bond twice)."""
    s = np.asarray(spins)
    shape3, per = lattice(s.shape, periodic)
    return p3.measure(s.reshape(shape3), q, per)


def _site_terms(spins, q, periodic, J, h):
    """l of every site in index order: h[s_i][i], then + J_right, + J_down, + J_layer of its bonds that exist and join two equal
    colours (one rounded add each)."""
    s0 = np.asarray(spins, dtype=np.int8)
    shape3, per = lattice(s0.shape, periodic)
    jr, jd, jl, hh = as_disorder(s0.shape, periodic, J, h, q)
    s = s0.reshape(shape3).astype(np.int64)
    where = np.indices(shape3)
    if hh is None:
        l = np.zeros(shape3, np.float64)
    else:
        l = np.take_along_axis(hh.astype(np.float64), s[None], axis=0)[0]
    for axis, Jb in ((2, jr), (1, jd), (0, jl)):
        has = np.ones(shape3, bool) if per[axis] else where[axis] < shape3[axis] - 1
        eq = has & (s == np.roll(s, -1, axis))
        l = np.where(eq, l + Jb.astype(np.float64), l)
    return l.ravel()


def _tree256(e):
    """block_sum of reduce_dev.h over the last axis of 256 lanes: a shuffle tree per wave of 64, then (w0 + w1) + (w2 + w3)."""
    v = e.reshape(e.shape[:-1] + (4, 64))
    for off in (32, 16, 8, 4, 2, 1):
        v = v[..., :off] + v[..., off:2 * off]
    w = v[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def _strided_sum(x, lanes):
    """Lane g adds x[g], x[g + lanes], .. in this order, starting from 0.0: (lanes,) float64."""
    k = -(-x.size // lanes)
    pad = np.zeros(k * lanes, np.float64)
    pad[:x.size] = x
    e = np.zeros(lanes, np.float64)
    for row in pad.reshape(k, lanes):
        e = e + row
    return e


def energy(spins, q, periodic, J, h=None):
    """E in the device's fixed order (k12_measure's partials, energy_final): the bits of tsu_potts_dis_measure's E."""
    l = _site_terms(spins, q, periodic, J, h)
    blocks = min(-(-l.size // 256), 1024)
    part = _tree256(_strided_sum(l, blocks * 256).reshape(blocks, 256))
    return float(-_tree256(_strided_sum(part, 256)))


def energy_plain(spins, q, periodic, J, h=None):
    """The same energy as one math.fsum."""
    return -math.fsum(_site_terms(spins, q, periodic, J, h).tolist())


def boltzmann_chi2(codes, shape, q, periodic, J, h, T):
    """chi^2 of the histogram of `codes` against exp(-E / T) / Z over the q^N states: the states with expected count >= 5 one cell
    each, the rest pooled into one cell.  Returns (chi2, dof, p, pooled share of the probability)."""
    from scipy.stats import chi2 as chi2_dist
    shape3, per = lattice(shape, periodic)
    jr, jd, jl, hh = as_disorder(shape, periodic, J, h, q)
    n_sites = int(np.prod(shape3))
    n_states = int(q) ** n_sites
    k = np.arange(n_states, dtype=np.int64)
    digits = np.stack([(k // int(q) ** i) % int(q) for i in range(n_sites)], axis=1).reshape((n_states,) + shape3)
    E = np.zeros(n_states)
    for axis, Jb in ((2, jr), (1, jd), (0, jl)):
        ax = axis + 1
        eq = digits == np.roll(digits, -1, ax)
        Jm = Jb.astype(np.float64).copy()
        if not per[axis]:
            edge = [slice(None)] * 3
            edge[axis] = -1
            Jm[tuple(edge)] = 0.0
        E -= (eq * Jm[None]).sum(axis=(1, 2, 3))
    if hh is not None:
        E -= np.take_along_axis(np.broadcast_to(hh.astype(np.float64)[None], (n_states,) + hh.shape), digits[:, None], axis=1)[:, 0].sum(axis=(1, 2, 3))
    w = np.exp(-(E - E.min()) / float(T))
    prob = w / w.sum()
    expected = len(codes) * prob
    counts = np.bincount(np.asarray(codes, dtype=np.int64), minlength=n_states).astype(np.float64)
    big = expected >= 5.0
    obs = np.append(counts[big], counts[~big].sum())
    exp = np.append(expected[big], expected[~big].sum())
    keep = exp > 0
    chi2 = float(np.sum((obs[keep] - exp[keep]) ** 2 / exp[keep]))
    dof = int(np.count_nonzero(keep)) - 1
    return chi2, dof, float(chi2_dist.sf(chi2, dof)), float(prob[~big].sum())


# ---------------------------------------------------------------- long chains of tiny lattices, in plain Python floats
def _site_bonds(shape3, per, jr, jd, jl):
    """Per site: [(neighbour index, coupling)] of its existing neighbours in the contract's order."""
    D, R, C = shape3
    Js = {0: jl.astype(np.float64), 1: jd.astype(np.float64), 2: jr.astype(np.float64)}
    out = []
    for z in range(D):
        for r in range(R):
            for c in range(C):
                nb = []
                for axis, d in ((0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1)):
                    p = [z, r, c]
                    p[axis] += d
                    if per[axis]:
                        p[axis] %= shape3[axis]
                    elif not 0 <= p[axis] < shape3[axis]:
                        continue
                    at = tuple(p) if d == -1 else (z, r, c)  # where the bond is stored
                    nb.append(((p[0] * R + p[1]) * C + p[2], float(Js[axis][at])))
                out.append(nb)
    return out


def chain(spins, q, periodic, J, h, T, n_sweeps, seed, sweep0=0, replica=0, record_every=0, block=4096):
    """n_sweeps heat-bath sweeps of a tiny lattice in plain Python arithmetic.  Returns (final int8 array, codes, fragile decisions):
    the state_code after every record_every-th sweep (none if 0).  Equal to `sweep` bit for bit."""
    s0 = np.array(spins, dtype=np.int8)
    shape3, per = lattice(s0.shape, periodic)
    jr, jd, jl, hh = as_disorder(s0.shape, periodic, J, h, q)
    n = s0.size
    nbs = _site_bonds(shape3, per, jr, jd, jl)
    h_of = [[0.0] * q for _ in range(n)] if hh is None else hh.astype(np.float64).reshape(q, n).T.tolist()
    col_of = p3.colours(shape3).ravel().tolist()
    of_colour = [[i for i in range(n) if col_of[i] == col] for col in (0, 1)]
    s = s0.ravel().tolist()
    powers = [int(q) ** i for i in range(n)]
    T = float(T)
    codes, done, n_fragile = [], 0, 0
    while done < n_sweeps:
        nb_sweeps = min(block, n_sweeps - done)
        U = p3._uniform_block(shape3, int(sweep0) + done, nb_sweeps, seed, replica)
        for k in range(nb_sweeps):
            for col in (0, 1):
                u_row = U[2 * k + col]
                for i in of_colour[col]:
                    a = list(h_of[i])
                    for j, Jk in nbs[i]:
                        a[s[j]] += Jk
                    amax = max(a)
                    Z, acc = [], 0.0
                    for c in range(q):
                        w = math.exp((a[c] - amax) / T)
                        acc = w if c == 0 else acc + w
                        Z.append(acc)
                    u = u_row[i]
                    new = q - 1
                    for c in range(q - 2, -1, -1):
                        real = Z[c] / acc * TWO32
                        if abs(u - real) <= 1.0:
                            n_fragile += 1
                        if u < math.floor(real + 0.5):
                            new = c
                    s[i] = new
            done += 1
            if record_every and done % record_every == 0:
                codes.append(sum(v * p for v, p in zip(s, powers)))
    return np.array(s, np.int8).reshape(s0.shape), codes, n_fragile


def cluster_chain(spins, q, periodic, J, T, n_steps, seed, step0=0, replica=0, record_every=0, block=4096):
    """n_steps Swendsen-Wang steps of a tiny lattice in plain Python integers.  Returns (final int8 array, codes, fragile decisions).
    Equal to `cluster_sweep` bit for bit."""
    s0 = np.array(spins, dtype=np.int8)
    shape3, per = lattice(s0.shape, periodic)
    jr, jd, jl, _ = as_disorder(s0.shape, periodic, J)
    D, R, C = shape3
    n = s0.size
    T = float(T)
    bonds = []  # (site, neighbour, which of the site's three bond words, threshold, real-valued threshold)
    for z in range(D):
        for r in range(R):
            for c in range(C):
                i = (z * R + r) * C + c
                for d, (has, j, Jb) in enumerate((((c + 1 < C or per[2]), (z * R + r) * C + (c + 1) % C, jr),
                                                  ((r + 1 < R or per[1]), (z * R + (r + 1) % R) * C + c, jd),
                                                  ((z + 1 < D or per[0]), (((z + 1) % D) * R + r) * C + c, jl))):
                    if has:
                        real = -math.expm1(-float(Jb[z, r, c]) / T) * TWO32
                        bonds.append((i, j, d, math.floor(real), real))
    rho = np.repeat(np.arange(D * R), C)
    Cc = np.tile(np.arange(C), D * R)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    s = s0.ravel().tolist()
    powers = [int(q) ** i for i in range(n)]
    codes, done, n_fragile = [], 0, 0
    while done < n_steps:
        nb = min(block, n_steps - done)
        t = (int(step0) + done + np.arange(nb, dtype=np.uint64))[:, None]
        Wb = np.stack(philox4x32_10((Cc >> 1)[None, :], rho[None, :], t, p3.TAG_SW_BOND | (int(replica) << 8), k0, k1))
        Wl = np.stack(philox4x32_10((Cc >> 2)[None, :], rho[None, :], t, p3.TAG_SW_LAYER | (int(replica) << 8), k0, k1))
        Wf = np.stack(philox4x32_10((Cc >> 2)[None, :], rho[None, :], t, p3.TAG_SW_FLIP | (int(replica) << 8), k0, k1))
        sel = np.arange(n)[None, :]
        steps = np.arange(nb)[:, None]
        u_bond = [Wb[(2 * (Cc & 1) + d)[None, :], steps, sel].tolist() for d in (0, 1)] + [Wl[(Cc & 3)[None, :], steps, sel].tolist()]
        w_flip = Wf[(Cc & 3)[None, :], steps, sel].tolist()
        for k in range(nb):
            parent = list(range(n))

            def find(x):
                while parent[x] != x:
                    x = parent[x]
                return x
            for i, j, d, thr, real in bonds:
                if s[i] == s[j]:
                    u = u_bond[d][k][i]
                    if abs(u - real) <= 1.0:
                        n_fragile += 1
                    if u < thr:
                        a, b = find(i), find(j)
                        if a != b:
                            parent[max(a, b)] = min(a, b)
            s = [(w_flip[k][find(i)] * q) >> 32 for i in range(n)]
            done += 1
            if record_every and done % record_every == 0:
                codes.append(sum(v * p for v, p in zip(s, powers)))
    return np.array(s, np.int8).reshape(s0.shape), codes, n_fragile


# ---------------------------------------------------------------- the cases of tests/test_potts_disorder_gpu.py
# Every bit-for-bit GPU case is listed here so that tests/test_potts_disorder_cpu.py can assert, without a device, that none of
# them holds a fragile decision.  3 sweeps or steps each.
N_UPDATES = 3
SEEDS = (2 ** 64 - 59, 0x9E3779B97F4A7C15, 12345)
# open 5 x 19: scalar loads, a partial octet; periodic 6 x 32: whole octets, two a row, both wraps; periodic 2 x 2 and 2 x 4 x 16:
# double bonds with two different couplings; open 3 x 5 x 7; periodic 4 x 4 x 16
HEAT_BATH_SHAPES = [((5, 19), False), ((6, 32), True), ((2, 2), True), ((2, 4, 16), True), ((3, 5, 7), False), ((4, 4, 16), True)]
# couplings from {0, 1, 2}: 8 x 12 on one workgroup and on tiles of edge 4, 4 x 6 x 8 on one workgroup and on 2 x 3 x 4 tiles, open
# and with every wrap
CLUSTER_SHAPES = [((8, 12), False), ((8, 12), True), ((4, 6, 8), False), ((4, 6, 8), True)]


def heat_bath_cases():
    out = []
    for i, (shape, per) in enumerate(HEAT_BATH_SHAPES):
        for j, q in enumerate((2, 3, 8)):
            for field in (False, True):
                k = len(out)
                out.append(dict(shape=shape, periodic=per, q=q, field=field, T=(0.7, 1.3, 2.5)[k % 3], seed=SEEDS[k % 3],
                                sweep0=(0, 2 ** 32 - 1)[(i + j) % 2], replica=(0, 3)[(k // 2) % 2], dseed=100 + k, kind="gaussian"))
    return out


def cluster_cases():
    out = []
    for i, (shape, per) in enumerate(CLUSTER_SHAPES):
        for q in (2, 3, 8):
            k = len(out)
            out.append(dict(shape=shape, periodic=per, q=q, field=False, T=(0.9, 1.5, 2.5)[k % 3], seed=SEEDS[k % 3], sweep0=(0, 77)[k % 2],
                            replica=(0, 5)[(k // 2) % 2], dseed=200 + k, kind="012"))
    return out


def case_id(case):
    per = case["periodic"]
    return "x".join(map(str, case["shape"])) + ("-p" if per else "-o") + f"-q{case['q']}" + ("-h" if case["field"] else "")


def case_inputs(case):
    """(spins, J, h) of a case, from its disorder seed."""
    rng = np.random.default_rng(case["dseed"])
    spins = rng.integers(0, case["q"], size=case["shape"]).astype(np.int8)
    J, h = random_disorder(case["shape"], case["periodic"], case["q"], rng, case["kind"], case["field"])
    return spins, J, h


# The enumeration table of the contract, every lattice started from colour 0 (K10's protocol: 100 updates discarded, 20 000 states 4
# updates apart): (shape, q, periodic, kind of couplings, with a site field, T, disorder seed, chain seed)
ENUMERATION_HEAT_BATH = [((2, 3), 3, False, "gaussian", True, 1.5, 11, 5000), ((2, 2, 2), 2, False, "gaussian", True, 2.0, 12, 5001)]
ENUMERATION_CLUSTER = [((2, 3), 3, False, "012", False, 1.5, 13, 6000)]
N_DISCARD, N_STATES, EVERY = 100, 20000, 4


def enumeration_disorder(case):
    shape, q, per, kind, field, T, dseed, seed = case
    return random_disorder(shape, per, q, np.random.default_rng(dseed), kind, field)

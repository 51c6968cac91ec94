"""NumPy twin of K10 on the cubic lattice (csrc/potts3d.hip, csrc/potts_dev.h), bit for bit.

State: (D, R, C) int8 colours 0 .. q - 1; periodic = (p_z, p_r, p_c) (a bool means all three).  E = -J n_eq - sum_c h_c N_c over the
bonds of three axes; a periodic axis of length 2 counts its double bond twice.  Global row rho = z R + r, site index i = rho C + c.

Heat bath, half-sweep hs = 2 sweep + colour (32-bit words), colour = (z + r + c) & 1, key = seed:
  u     potts_twin's site uniform with rho in place of r: site_uniforms(D R, C, hs, seed, replica).reshape(D, R, C)
  E[n]  = exp(J n / T), n = 0 .. 6; F[c] = exp(h_c / T): math.exp
  w_c   = E[n_c] F[c], n_c the existing neighbours (up to six) of colour c; Z_c and the pick are potts_twin's
Swendsen-Wang step t (J > 0, zero field):
  bond  right and down bonds of (z, r, c): words 2 (c & 1) and 2 (c & 1) + 1 of Philox(c >> 1, rho, t, TAG_SW_BOND | replica << 8);
        the layer bond to z + 1 (to z = 0 across a periodic z): word c & 3 of Philox(c >> 2, rho, t, TAG_SW_LAYER | replica << 8);
        active iff the two colours are equal and u < thr, thr = potts_twin.threshold(J, T)
  label the smallest site index of the component
  new colour of the cluster rooted at (rho, c): (W q) >> 32, W = word c & 3 of Philox(c >> 2, rho, t, TAG_SW_FLIP | replica << 8)
On (1, R, C) with periodic (False, p, p) everything here equals potts_twin on (R, C).

`sweep` and `cluster_step` are vectorised over the sites; `chain` and `cluster_chain` run long chains of tiny lattices in plain Python
floats and integers (the same IEEE operations, no fused multiply-add).
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


_p2 = _load("potts_twin")
philox4x32_10 = _p2.philox4x32_10
site_uniforms_2d = _p2.site_uniforms
threshold, pick, cumulative, order_parameter = _p2.threshold, _p2.pick, _p2.cumulative, _p2.order_parameter
TAG_ISING_HI, TAG_ISING_LO, TAG_SW_BOND, TAG_SW_FLIP, TAG_SW_LAYER = 0, 1, 6, 7, 10
MAX_Q = 8
TWO32 = 4294967296.0
OPEN, ALL = (False, False, False), (True, True, True)

# The enumeration table of the contract, every lattice started from colour 0:
# (shape, q, periodic, J, h, T, states recorded, chain seed) for heat-bath sweeps, the same without h for Swendsen-Wang steps
ENUMERATION_HEAT_BATH = [((2, 2, 2), 2, OPEN, 1.0, (0.0, 0.25), 2.5, 20000, 3000),
                         ((2, 2, 2), 2, (True, False, False), 1.0, None, 4.0, 20000, 3001),
                         ((2, 2, 2), 2, ALL, 0.5, (0.1, -0.1), 4.0, 20000, 3002),
                         ((2, 2, 2), 2, OPEN, -1.0, (0.0, 0.25), 2.0, 20000, 3003),
                         ((2, 1, 3), 3, OPEN, 1.0, None, 1.5, 20000, 3004)]
ENUMERATION_HEAT_BATH_LONG = ((2, 2, 2), 3, OPEN, 1.0, None, 2.5, 100000, 3005)  # the CPU file only
ENUMERATION_CLUSTER = [((2, 1, 3), 3, OPEN, 1.0, 1.5, 20000, 4000), ((2, 2, 2), 2, OPEN, 1.0, 2.5, 20000, 4001)]


def axes(periodic):
    """(p_z, p_r, p_c) from a bool or a triple."""
    if isinstance(periodic, (bool, np.bool_)):
        return (bool(periodic),) * 3
    p = tuple(bool(x) for x in periodic)
    assert len(p) == 3
    return p


def check_model(q, J, h, T):
    """The refusals of the contract (the six-neighbour bound, whatever the depth); returns h as a list of q floats."""
    if not 2 <= int(q) <= MAX_Q:
        raise ValueError("q must be in 2 .. 8")
    hh = [0.0] * int(q) if h is None else [float(v) for v in h]
    if len(hh) != int(q):
        raise ValueError("h must hold q values")
    if not all(math.isfinite(v) for v in [float(J), float(T)] + hh):
        raise ValueError("J, h and T must be finite")
    if not T > 0:
        raise ValueError("Temperature must be positive")
    if (6.0 * abs(float(J)) + max(hh) - min(hh)) / float(T) > 600.0:
        raise ValueError("(6 |J| + max h - min h) / T exceeds 600")
    return hh


def tables(q, J, h, T):
    """(E[0 .. 6], F[0 .. q - 1]) as float64 arrays."""
    hh = check_model(q, J, h, T)
    J, T = float(J), float(T)
    return (np.array([math.exp(J * float(n) / T) for n in range(7)]), np.array([math.exp(v / T) for v in hh]))


def neighbours(s, periodic):
    """The six neighbour colours of every site (z - 1, z + 1, r - 1, r + 1, c - 1, c + 1) as int64 arrays, -1 where an open axis has
    none."""
    s = np.asarray(s, dtype=np.int64)
    out = []
    for axis, p in enumerate(axes(periodic)):
        for shift in (1, -1):
            nb = np.roll(s, shift, axis).copy()
            if not p:
                edge = [slice(None)] * 3
                edge[axis] = 0 if shift == 1 else -1
                nb[tuple(edge)] = -1
            out.append(nb)
    return out


def colours(shape):
    D, R, C = shape
    return (np.arange(D)[:, None, None] + np.arange(R)[None, :, None] + np.arange(C)[None, None, :]) & 1


def site_uniforms(shape, hs, seed, replica=0):
    D, R, C = shape
    return site_uniforms_2d(D * R, C, hs, seed, replica).reshape(D, R, C)


def sweep(spins, q, periodic, J, h, T, n_sweeps, seed, sweep0=0, replica=0):
    """n_sweeps heat-bath sweeps; returns a new int8 array."""
    s = np.array(spins, dtype=np.int8)
    assert s.ndim == 3
    E, F = tables(q, J, h, T)
    colour_of = colours(s.shape)
    for k in range(int(n_sweeps)):
        sw = (int(sweep0) + k) & 0xFFFFFFFF
        for colour in (0, 1):
            hs = (2 * sw + colour) & 0xFFFFFFFF
            u = site_uniforms(s.shape, hs, seed, replica)
            nb = neighbours(s, periodic)
            counts = [sum((x == c).astype(np.int64) for x in nb) for c in range(q)]
            new = pick(cumulative(E, F, counts), u)
            s = np.where(colour_of == colour, new, s).astype(np.int8)
    return s


# ---------------------------------------------------------------- the sites the low half of u decides (potts_twin.lo_mask)
lo_mask, lo_octets, lo_fold = _p2.lo_mask, _p2.lo_octets, _p2.lo_fold  # octets of global rows: the masks fold as (D R, C)


def lo_decided(spins, q, periodic, J, h, T, hs, seed, replica=0):
    """The boolean mask of the sites of half-sweep hs (colour hs & 1) of `spins` that the low half of u decides."""
    s = np.array(spins, dtype=np.int8)
    assert s.ndim == 3
    E, F = tables(q, J, h, T)
    hs = int(hs) & 0xFFFFFFFF
    nb = neighbours(s, periodic)
    counts = [sum((x == c).astype(np.int64) for x in nb) for c in range(q)]
    return lo_mask(cumulative(E, F, counts), site_uniforms(s.shape, hs, seed, replica)) & (colours(s.shape) == (hs & 1))


def lo_trajectory(spins, q, periodic, J, h, T, n_sweeps, seed, sweep0=0, replica=0):
    """`sweep` half-sweep by half-sweep: (the final state, the lo_decided mask of each of the 2 n_sweeps half-sweeps in order)."""
    s = np.array(spins, dtype=np.int8)
    assert s.ndim == 3
    E, F = tables(q, J, h, T)
    colour_of = colours(s.shape)
    masks = []
    for k in range(int(n_sweeps)):
        for colour in (0, 1):
            hs = (2 * ((int(sweep0) + k) & 0xFFFFFFFF) + colour) & 0xFFFFFFFF
            u = site_uniforms(s.shape, hs, seed, replica)
            nb = neighbours(s, periodic)
            Z = cumulative(E, F, [sum((x == c).astype(np.int64) for x in nb) for c in range(q)])
            masks.append(lo_mask(Z, u) & (colour_of == colour))
            s = np.where(colour_of == colour, pick(Z, u), s).astype(np.int8)
    return s, masks


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
    wl = _words(seed, rho, c >> 2, int(t), TAG_SW_LAYER | (int(replica) << 8))
    return (np.where(odd, w[2], w[0]).astype(np.uint64), np.where(odd, w[3], w[1]).astype(np.uint64),
            np.choose(c & 3, wl).astype(np.uint64))


def labels(spins, periodic, J, T, seed, t, replica=0):
    """Root index of every site's cluster, (D, R, C) int64."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    s = np.asarray(spins, dtype=np.int64)
    shape, n = s.shape, s.size
    per = axes(periodic)
    thr = np.uint64(threshold(J, T))
    us = bond_uniforms(shape, seed, t, replica)
    where = np.indices(shape)
    idx = np.arange(n, dtype=np.int64).reshape(shape)
    src, dst = [], []
    for axis, u in ((2, us[0]), (1, us[1]), (0, us[2])):
        has = np.ones(shape, bool) if per[axis] else where[axis] < shape[axis] - 1
        act = has & (s == np.roll(s, -1, axis)) & (u < thr)
        src.append(idx[act])
        dst.append(np.roll(idx, -1, axis)[act])
    src, dst = np.concatenate(src), np.concatenate(dst)
    g = coo_matrix((np.ones(src.size, np.int8), (src, dst)), shape=(n, n))
    ncomp, lab = connected_components(g, directed=False)
    root = np.full(ncomp, n, dtype=np.int64)
    np.minimum.at(root, lab, np.arange(n, dtype=np.int64))
    return root[lab].reshape(shape)


def cluster_step(spins, q, periodic, J, T, seed, t, replica=0):
    """One Swendsen-Wang step; returns a new int8 array."""
    s = np.asarray(spins, dtype=np.int8)
    cols = s.shape[2]
    roots = labels(s, periodic, J, T, seed, t, replica)
    u = np.unique(roots)
    rho, rc = u // cols, u % cols
    w = _words(seed, rho, rc >> 2, int(t), TAG_SW_FLIP | (int(replica) << 8))
    word = np.choose((rc & 3).astype(np.int64), w).astype(np.uint64)
    colour = ((word * np.uint64(q)) >> np.uint64(32)).astype(np.int8)
    return colour[np.searchsorted(u, roots)].astype(np.int8)


def cluster_sweep(spins, q, periodic, J, T, n_steps, seed, step0=0, replica=0):
    s = np.asarray(spins, dtype=np.int8)
    for k in range(int(n_steps)):
        s = cluster_step(s, q, periodic, J, T, seed, int(step0) + k, replica)
    return s


def _n_eq(s, periodic, lead=0):
    """Equal bonds over the last three axes of s (`lead` leading axes are kept)."""
    total = 0
    for axis, p in enumerate(axes(periodic)):
        ax = lead + axis
        if p:
            eq = s == np.roll(s, -1, ax)
        else:
            a = [slice(None)] * s.ndim
            b = [slice(None)] * s.ndim
            a[ax], b[ax] = slice(None, -1), slice(1, None)
            eq = s[tuple(a)] == s[tuple(b)]
        total = total + eq.sum(axis=tuple(range(lead, s.ndim)))
    return total


def measure(spins, q, periodic):
    """(n_eq, N_0 .. N_{q-1}): exact integers; a periodic axis of length 2 counts its double bond twice."""
    s = np.asarray(spins, dtype=np.int64)
    assert s.ndim == 3
    return int(_n_eq(s, periodic)), np.bincount(s.ravel(), minlength=q).astype(np.int64)


def energy(spins, q, periodic, J, h=None):
    n_eq, N = measure(spins, q, periodic)
    hh = np.zeros(q) if h is None else np.asarray(h, dtype=np.float64)
    return -float(J) * n_eq - float(np.dot(hh, N))


def state_code(s, q):
    """The state as an integer: digit i (base q) = the colour of site i (row-major)."""
    return _p2.state_code(s, q)


def boltzmann_chi2(codes, shape, q, periodic, J, h, T):
    """chi^2 of the histogram of `codes` against exp(-E / T) / Z over the q^N states: the states with expected count >= 5 one cell
    each, the rest pooled into one cell.  Returns (chi2, dof, p, pooled share of the probability)."""
    from scipy.stats import chi2 as chi2_dist
    n_sites = int(np.prod(shape))
    n_states = int(q) ** n_sites
    k = np.arange(n_states, dtype=np.int64)
    digits = np.stack([(k // int(q) ** i) % int(q) for i in range(n_sites)], axis=1).reshape((n_states,) + tuple(shape))
    n_eq = _n_eq(digits, periodic, lead=1)
    hh = np.zeros(q) if h is None else np.asarray(h, dtype=np.float64)
    E = -float(J) * n_eq - hh[digits].sum(axis=(1, 2, 3))
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


# ---------------------------------------------------------------- long chains of tiny lattices
def _site_lists(shape, periodic):
    """Per site: the list of its existing neighbours' indices (a periodic axis of length 2 lists its neighbour twice)."""
    D, R, C = shape
    per = axes(periodic)
    out = []
    for z in range(D):
        for r in range(R):
            for c in range(C):
                nb = []
                for axis, d in ((0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1)):
                    p = [z, r, c]
                    p[axis] += d
                    if per[axis]:
                        p[axis] %= shape[axis]
                    elif not 0 <= p[axis] < shape[axis]:
                        continue
                    nb.append((p[0] * R + p[1]) * C + p[2])
                out.append(nb)
    return out


def _uniform_block(shape, sweep_first, n_sweeps, seed, replica):
    """u of the half-sweeps of sweeps sweep_first .. sweep_first + n_sweeps - 1: (2 n_sweeps, D R C) Python ints."""
    D, R, C = shape
    hs = (2 * ((int(sweep_first) + np.arange(n_sweeps, dtype=np.uint64)) & np.uint64(0xFFFFFFFF))[:, None]
          + np.arange(2, dtype=np.uint64)[None, :]).reshape(-1) & np.uint64(0xFFFFFFFF)
    rho = np.repeat(np.arange(D * R), C)
    c = np.tile(np.arange(C), D * R)
    m = (c >> 1) & 7
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    halves = []
    for tag in (TAG_ISING_HI, TAG_ISING_LO):
        W = np.stack(philox4x32_10((c >> 4)[None, :], rho[None, :], hs[:, None], tag | (int(replica) << 8), k0, k1))  # (4, n_hs, n)
        word = W[(m >> 1)[None, :], np.arange(len(hs))[:, None], np.arange(rho.size)[None, :]]
        halves.append((word >> (16 * (m & 1)).astype(np.uint32)[None, :]) & np.uint32(0xFFFF))
    hi = halves[0] ^ np.uint32(0x8000)
    return ((hi.astype(np.uint64) << np.uint64(16)) | halves[1].astype(np.uint64)).tolist()


def chain(spins, q, periodic, J, h, T, n_sweeps, seed, sweep0=0, replica=0, record_every=0, block=4096):
    """n_sweeps heat-bath sweeps of a tiny lattice in plain Python arithmetic.  Returns (final int8 array, codes): the state_code
    after every record_every-th sweep (none if 0).  Equal to `sweep` bit for bit (tests/test_potts3d_cpu.py compares them)."""
    s0 = np.array(spins, dtype=np.int8)
    shape = s0.shape
    n = s0.size
    E, F = (a.tolist() for a in tables(q, J, h, T))
    nbs = _site_lists(shape, periodic)
    col_of = colours(shape).ravel().tolist()
    of_colour = [[i for i in range(n) if col_of[i] == col] for col in (0, 1)]
    s = s0.ravel().tolist()
    powers = [int(q) ** i for i in range(n)]
    codes = []
    done = 0
    while done < n_sweeps:
        nb_sweeps = min(block, n_sweeps - done)
        U = _uniform_block(shape, int(sweep0) + done, nb_sweeps, seed, replica)
        for k in range(nb_sweeps):
            for col in (0, 1):
                u_row = U[2 * k + col]
                for i in of_colour[col]:
                    cnt = [0] * q
                    for j in nbs[i]:
                        cnt[s[j]] += 1
                    Z = []
                    acc = 0.0
                    for c in range(q):
                        w = E[cnt[c]] * F[c]
                        acc = w if c == 0 else acc + w
                        Z.append(acc)
                    lhs = float(u_row[i]) * Z[q - 1]
                    new = q - 1
                    for c in range(q - 1):
                        if lhs < Z[c] * TWO32:
                            new = c
                            break
                    s[i] = new
            done += 1
            if record_every and done % record_every == 0:
                codes.append(sum(v * p for v, p in zip(s, powers)))
    return np.array(s, np.int8).reshape(shape), codes


def cluster_chain(spins, q, periodic, J, T, n_steps, seed, step0=0, replica=0, record_every=0, block=4096):
    """n_steps Swendsen-Wang steps of a tiny lattice in plain Python integers.  Returns (final int8 array, codes).  Equal to
    `cluster_sweep` bit for bit."""
    s0 = np.array(spins, dtype=np.int8)
    shape = s0.shape
    D, R, C = shape
    n = s0.size
    per = axes(periodic)
    thr = threshold(J, T)
    bonds = []  # (site, neighbour, which of the site's three bond words: right, down, layer)
    for z in range(D):
        for r in range(R):
            for c in range(C):
                i = (z * R + r) * C + c
                if c + 1 < C or per[2]:
                    bonds.append((i, (z * R + r) * C + (c + 1) % C, 0))
                if r + 1 < R or per[1]:
                    bonds.append((i, (z * R + (r + 1) % R) * C + c, 1))
                if z + 1 < D or per[0]:
                    bonds.append((i, (((z + 1) % D) * R + r) * C + c, 2))
    rho = np.repeat(np.arange(D * R), C)
    Cc = np.tile(np.arange(C), D * R)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    s = s0.ravel().tolist()
    powers = [int(q) ** i for i in range(n)]
    codes = []
    done = 0
    while done < n_steps:
        nb = min(block, n_steps - done)
        t = (int(step0) + done + np.arange(nb, dtype=np.uint64))[:, None]
        Wb = np.stack(philox4x32_10((Cc >> 1)[None, :], rho[None, :], t, TAG_SW_BOND | (int(replica) << 8), k0, k1))
        Wl = np.stack(philox4x32_10((Cc >> 2)[None, :], rho[None, :], t, TAG_SW_LAYER | (int(replica) << 8), k0, k1))
        Wf = np.stack(philox4x32_10((Cc >> 2)[None, :], rho[None, :], t, TAG_SW_FLIP | (int(replica) << 8), k0, k1))
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
            for i, j, d in bonds:
                if s[i] == s[j] and u_bond[d][k][i] < thr:
                    a, b = find(i), find(j)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
            s = [(w_flip[k][find(i)] * q) >> 32 for i in range(n)]
            done += 1
            if record_every and done % record_every == 0:
                codes.append(sum(v * p for v, p in zip(s, powers)))
    return np.array(s, np.int8).reshape(shape), codes

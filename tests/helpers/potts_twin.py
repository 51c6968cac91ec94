"""NumPy twin of K10, the q-state Potts lattice (csrc/potts2d.hip, csrc/potts_dev.h), bit for bit.

State: (rows, cols) int8 colours 0 .. q - 1.  E = -J n_eq - sum_c h_c N_c.

Heat bath, half-sweep hs = 2 sweep + colour (32-bit words), colour = (r + c) & 1, key = seed:
  u     K1's 32-bit site uniform exactly as K7 uses it (disorder_twin.site_uniforms)
  E[n]  = exp(J n / T), n = 0 .. 4; F[c] = exp(h_c / T): math.exp, the C library's exp the host side of the device uses
  w_c   = E[n_c] F[c], n_c the existing neighbours of colour c (one rounded multiply)
  Z_c   = Z_{c-1} + w_c in colour order, Z_0 = w_0 (one rounded add each)
  new colour: the smallest c with float64(u) Z_{q-1} < Z_c 2^32, else q - 1
Swendsen-Wang step t (J > 0, zero field):
  bond  right bond of (r, c): word 2 (c & 1) of Philox(c >> 1, r, t, TAG_SW_BOND | replica << 8), down bond: word 2 (c & 1) + 1;
        active iff the two colours are equal and u < thr, thr = floor(-expm1(-J / T) 2^32)
  label the smallest site index of the component
  new colour of the cluster rooted at (r, c): (W q) >> 32, W = word c & 3 of Philox(c >> 2, r, t, TAG_SW_FLIP | replica << 8)

`sweep` and `cluster_step` are vectorised over the sites (any lattice); `chain` runs long chains of tiny lattices in plain Python
floats and integers (the same IEEE operations, no fused multiply-add) with the Philox blocks of many sweeps drawn at once.
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


_ct = _load("cluster_twin")
_dt = _load("disorder_twin")
philox4x32_10 = _ct.philox4x32_10
site_uniforms = _dt.site_uniforms
TAG_ISING_HI, TAG_ISING_LO, TAG_SW_BOND, TAG_SW_FLIP = 0, 1, 6, 7
MAX_Q = 8
TWO32 = 4294967296.0

# The enumeration table of the contract, all open lattices started from colour 0: (shape, q, J, T, h, chain seed) for heat-bath
# sweeps, (shape, q, J, T, chain seed) for Swendsen-Wang steps.  Open 2 x 2 with q = 8 is not here: it pools 43 % of the probability
ENUMERATION_HEAT_BATH = [((2, 3), 3, 1.0, 1.5, (0.3, 0.0, -0.2), 1000), ((2, 2), 5, 1.0, 1.2, None, 1001),
                         ((3, 3), 2, -1.0, 1.0, (0.0, 0.25), 1002), ((1, 3), 8, 1.0, 2.0, None, 1003)]
ENUMERATION_CLUSTER = [((2, 3), 3, 1.0, 1.5, 2000), ((2, 2), 5, 1.0, 1.2, 2001)]


def check_model(q, J, h, T):
    """The refusals of the contract; returns h as a list of q floats."""
    if not 2 <= int(q) <= MAX_Q:
        raise ValueError("q must be in 2 .. 8")
    hh = [0.0] * int(q) if h is None else [float(v) for v in h]
    if len(hh) != int(q):
        raise ValueError("h must hold q values")
    if not all(math.isfinite(v) for v in [float(J), float(T)] + hh):
        raise ValueError("J, h and T must be finite")
    if not T > 0:
        raise ValueError("Temperature must be positive")
    if (4.0 * abs(float(J)) + max(hh) - min(hh)) / float(T) > 600.0:
        raise ValueError("(4 |J| + max h - min h) / T exceeds 600")
    return hh


def tables(q, J, h, T):
    """(E[0 .. 4], F[0 .. q - 1]) as float64 arrays."""
    hh = check_model(q, J, h, T)
    J, T = float(J), float(T)
    return (np.array([math.exp(J * float(n) / T) for n in range(5)]), np.array([math.exp(v / T) for v in hh]))


def threshold(J, T):
    if not (T > 0 and J > 0):
        raise ValueError("the Potts cluster threshold needs J > 0 and T > 0")
    return int(math.floor(-math.expm1(-float(J) / float(T)) * TWO32))


def pick(Z, u):
    """Steps 3 - 4 for arrays: Z a list of q cumulative float64 arrays, u uint32; the colour as int8."""
    q = len(Z)
    lhs = u.astype(np.float64) * Z[q - 1]
    colour = np.full(np.shape(lhs), q - 1, np.int8)
    for c in range(q - 2, -1, -1):
        colour = np.where(lhs < Z[c] * TWO32, np.int8(c), colour)
    return colour


def cumulative(E, F, counts):
    """counts[c]: int arrays n_c -> the list Z_0 .. Z_{q-1}."""
    Z, acc = [], None
    for c in range(len(F)):
        w = E[counts[c]] * F[c]
        acc = w if acc is None else acc + w
        Z.append(acc)
    return Z


def neighbours(s, periodic):
    """(up, down, left, right) colours of every site as int64 arrays, -1 where an open lattice has none."""
    s = np.asarray(s, dtype=np.int64)
    up, dn, lf, rt = np.roll(s, 1, 0), np.roll(s, -1, 0), np.roll(s, 1, 1), np.roll(s, -1, 1)
    if not periodic:
        up, dn, lf, rt = up.copy(), dn.copy(), lf.copy(), rt.copy()
        up[0, :] = -1
        dn[-1, :] = -1
        lf[:, 0] = -1
        rt[:, -1] = -1
    return up, dn, lf, rt


def sweep(spins, q, periodic, J, h, T, n_sweeps, seed, sweep0=0, replica=0):
    """n_sweeps heat-bath sweeps; returns a new int8 array."""
    s = np.array(spins, dtype=np.int8)
    rows, cols = s.shape
    E, F = tables(q, J, h, T)
    colour_of = (np.arange(rows)[:, None] + np.arange(cols)[None, :]) & 1
    for k in range(int(n_sweeps)):
        sw = (int(sweep0) + k) & 0xFFFFFFFF
        for colour in (0, 1):
            hs = (2 * sw + colour) & 0xFFFFFFFF
            u = site_uniforms(rows, cols, hs, seed, replica)
            nb = neighbours(s, periodic)
            counts = [sum((x == c).astype(np.int64) for x in nb) for c in range(q)]
            new = pick(cumulative(E, F, counts), u)
            s = np.where(colour_of == colour, new, s).astype(np.int8)
    return s


# ---------------------------------------------------------------- the sites the low half of u decides
# The rule is monotone in u, so the kernels decide a site from the high half of u alone where the colour is the same at both ends
# of the 65536 values that share it, and draw the lo16 Philox block of the octet only for the others (potts_site, potts_site6).
def lo_mask(Z, u):
    """Z: the cumulative sums of every site, u: its uint32 uniform -> the sites whose colour differs between u & 0xFFFF0000 and
    u | 0xFFFF."""
    u = np.asarray(u, dtype=np.uint32)
    return pick(Z, u & np.uint32(0xFFFF0000)) != pick(Z, u | np.uint32(0xFFFF))


def lo_decided(spins, q, periodic, J, h, T, hs, seed, replica=0):
    """The boolean mask of the sites of half-sweep hs (colour hs & 1) of `spins` that the low half of u decides."""
    s = np.array(spins, dtype=np.int8)
    rows, cols = s.shape
    E, F = tables(q, J, h, T)
    hs = int(hs) & 0xFFFFFFFF
    nb = neighbours(s, periodic)
    counts = [sum((x == c).astype(np.int64) for x in nb) for c in range(q)]
    mine = ((np.arange(rows)[:, None] + np.arange(cols)[None, :]) & 1) == (hs & 1)
    return lo_mask(cumulative(E, F, counts), site_uniforms(rows, cols, hs, seed, replica)) & mine


def lo_octets(mask):
    """mask: (..., cols) booleans -> (global rows, octets) int64: the marked sites of every octet (16 columns of a global row)."""
    mask = np.asarray(mask, dtype=bool)
    cols = mask.shape[-1]
    noct = (cols + 15) >> 4
    wide = np.zeros((mask.size // cols, 16 * noct), np.int64)
    wide[:, :cols] = mask.reshape(-1, cols)
    return wide.reshape(-1, noct, 16).sum(axis=2)


def lo_fold(mask):
    """(the marked sites per octet position m = (c >> 1) & 7 as 8 ints, the number of octets that hold at least two of them)."""
    mask = np.asarray(mask, dtype=bool)
    m = (np.arange(mask.shape[-1]) >> 1) & 7
    per_m = [int(mask[..., m == k].sum()) for k in range(8)]
    return per_m, int((lo_octets(mask) >= 2).sum())


def lo_trajectory(spins, q, periodic, J, h, T, n_sweeps, seed, sweep0=0, replica=0):
    """`sweep` half-sweep by half-sweep: (the final state, the lo_decided mask of each of the 2 n_sweeps half-sweeps in order)."""
    s = np.array(spins, dtype=np.int8)
    rows, cols = s.shape
    E, F = tables(q, J, h, T)
    colour_of = (np.arange(rows)[:, None] + np.arange(cols)[None, :]) & 1
    masks = []
    for k in range(int(n_sweeps)):
        for colour in (0, 1):
            hs = (2 * ((int(sweep0) + k) & 0xFFFFFFFF) + colour) & 0xFFFFFFFF
            u = site_uniforms(rows, cols, hs, seed, replica)
            nb = neighbours(s, periodic)
            Z = cumulative(E, F, [sum((x == c).astype(np.int64) for x in nb) for c in range(q)])
            masks.append(lo_mask(Z, u) & (colour_of == colour))
            s = np.where(colour_of == colour, pick(Z, u), s).astype(np.int8)
    return s, masks


def _words(seed, r, c, t, tag):
    return philox4x32_10(c, r, t, tag, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)


def labels(spins, periodic, J, T, seed, t, replica=0):
    """Root index of every site's cluster, (rows, cols) int64."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    s = np.asarray(spins, dtype=np.int64)
    rows, cols = s.shape
    n = rows * cols
    thr = np.uint64(threshold(J, T))
    R, Cc = np.meshgrid(np.arange(rows, dtype=np.int64), np.arange(cols, dtype=np.int64), indexing="ij")
    w = _words(seed, R, Cc >> 1, int(t), TAG_SW_BOND | (int(replica) << 8))
    odd = (Cc & 1) == 1
    u_right = np.where(odd, w[2], w[0]).astype(np.uint64)
    u_down = np.where(odd, w[3], w[1]).astype(np.uint64)
    idx = np.arange(n, dtype=np.int64).reshape(rows, cols)
    ok_r = np.ones((rows, cols), bool) if periodic else (Cc < cols - 1)
    ok_d = np.ones((rows, cols), bool) if periodic else (R < rows - 1)
    act_r = ok_r & (s == np.roll(s, -1, 1)) & (u_right < thr)
    act_d = ok_d & (s == np.roll(s, -1, 0)) & (u_down < thr)
    src = np.concatenate([idx[act_r], idx[act_d]])
    dst = np.concatenate([np.roll(idx, -1, 1)[act_r], np.roll(idx, -1, 0)[act_d]])
    g = coo_matrix((np.ones(src.size, np.int8), (src, dst)), shape=(n, n))
    ncomp, lab = connected_components(g, directed=False)
    root = np.full(ncomp, n, dtype=np.int64)
    np.minimum.at(root, lab, np.arange(n, dtype=np.int64))
    return root[lab].reshape(rows, cols)


def cluster_step(spins, q, periodic, J, T, seed, t, replica=0):
    """One Swendsen-Wang step; returns a new int8 array."""
    s = np.asarray(spins, dtype=np.int8)
    rows, cols = s.shape
    roots = labels(s, periodic, J, T, seed, t, replica)
    u = np.unique(roots)
    rr, rc = u // cols, u % cols
    w = _words(seed, rr, rc >> 2, int(t), TAG_SW_FLIP | (int(replica) << 8))
    word = np.choose((rc & 3).astype(np.int64), w).astype(np.uint64)
    colour = ((word * np.uint64(q)) >> np.uint64(32)).astype(np.int8)
    return colour[np.searchsorted(u, roots)].astype(np.int8)


def cluster_sweep(spins, q, periodic, J, T, n_steps, seed, step0=0, replica=0):
    s = np.asarray(spins, dtype=np.int8)
    for k in range(int(n_steps)):
        s = cluster_step(s, q, periodic, J, T, seed, int(step0) + k, replica)
    return s


def measure(spins, q, periodic):
    """(n_eq, N_0 .. N_{q-1}): exact integers; a periodic axis of length 2 counts its double bond twice."""
    s = np.asarray(spins, dtype=np.int64)
    if periodic:
        n_eq = int(np.sum(s == np.roll(s, -1, 1)) + np.sum(s == np.roll(s, -1, 0)))
    else:
        n_eq = int(np.sum(s[:, :-1] == s[:, 1:]) + np.sum(s[:-1, :] == s[1:, :]))
    return n_eq, np.bincount(s.ravel(), minlength=q).astype(np.int64)


def energy(spins, q, periodic, J, h=None):
    n_eq, N = measure(spins, q, periodic)
    hh = np.zeros(q) if h is None else np.asarray(h, dtype=np.float64)
    return -float(J) * n_eq - float(np.dot(hh, N))


def order_parameter(N, q):
    N = np.asarray(N)
    return (q * N.max(axis=-1) / N.sum(axis=-1) - 1.0) / (q - 1.0)


def state_code(s, q):
    """The state as an integer: digit i (base q) = the colour of site i (row-major)."""
    code = 0
    for v in reversed(np.asarray(s).ravel().tolist()):
        code = code * int(q) + int(v)
    return code


def boltzmann_chi2(codes, shape, q, periodic, J, h, T):
    """chi^2 of the histogram of `codes` against exp(-E / T) / Z over the q^N states: the states with expected count >= 5 one cell
    each, the rest pooled into one cell.  Returns (chi2, dof, p, pooled share of the probability)."""
    from scipy.stats import chi2 as chi2_dist
    n_sites = int(np.prod(shape))
    n_states = int(q) ** n_sites
    k = np.arange(n_states, dtype=np.int64)
    digits = np.stack([(k // int(q) ** i) % int(q) for i in range(n_sites)], axis=1).reshape((n_states,) + tuple(shape))
    if periodic:
        n_eq = np.sum(digits == np.roll(digits, -1, 2), axis=(1, 2)) + np.sum(digits == np.roll(digits, -1, 1), axis=(1, 2))
    else:
        n_eq = np.sum(digits[:, :, :-1] == digits[:, :, 1:], axis=(1, 2)) + np.sum(digits[:, :-1, :] == digits[:, 1:, :], axis=(1, 2))
    hh = np.zeros(q) if h is None else np.asarray(h, dtype=np.float64)
    E = -float(J) * n_eq - hh[digits].sum(axis=(1, 2))
    w = np.exp(-(E - E.min()) / float(T))
    prob = w / w.sum()
    n = len(codes)
    expected = n * prob
    counts = np.bincount(np.asarray(codes, dtype=np.int64), minlength=n_states).astype(np.float64)
    big = expected >= 5.0
    obs = np.append(counts[big], counts[~big].sum())
    exp = np.append(expected[big], expected[~big].sum())
    keep = exp > 0
    chi2 = float(np.sum((obs[keep] - exp[keep]) ** 2 / exp[keep]))
    dof = int(np.count_nonzero(keep)) - 1
    return chi2, dof, float(chi2_dist.sf(chi2, dof)), float(prob[~big].sum())


# ---------------------------------------------------------------- long chains of tiny lattices
def _site_lists(rows, cols, periodic):
    """Per site: the list of its existing neighbours' indices (a periodic axis of length 2 lists its neighbour twice)."""
    out = []
    for r in range(rows):
        for c in range(cols):
            nb = []
            for rr, cc in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)):
                if periodic:
                    nb.append((rr % rows) * cols + cc % cols)
                elif 0 <= rr < rows and 0 <= cc < cols:
                    nb.append(rr * cols + cc)
            out.append(nb)
    return out


def _uniform_block(rows, cols, sweep_first, n_sweeps, seed, replica):
    """u of the half-sweeps of sweeps sweep_first .. sweep_first + n_sweeps - 1: (2 n_sweeps, rows * cols) Python ints, by one
    Philox call per tag."""
    hs = (2 * ((int(sweep_first) + np.arange(n_sweeps, dtype=np.uint64)) & np.uint64(0xFFFFFFFF))[:, None]
          + np.arange(2, dtype=np.uint64)[None, :]).reshape(-1) & np.uint64(0xFFFFFFFF)
    r = np.repeat(np.arange(rows), cols)
    c = np.tile(np.arange(cols), rows)
    m = (c >> 1) & 7
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    halves = []
    for tag in (TAG_ISING_HI, TAG_ISING_LO):
        W = np.stack(philox4x32_10((c >> 4)[None, :], r[None, :], hs[:, None], tag | (int(replica) << 8), k0, k1))  # (4, n_hs, n)
        word = W[(m >> 1)[None, :], np.arange(len(hs))[:, None], np.arange(r.size)[None, :]]
        halves.append((word >> (16 * (m & 1)).astype(np.uint32)[None, :]) & np.uint32(0xFFFF))
    hi = halves[0] ^ np.uint32(0x8000)
    return ((hi.astype(np.uint64) << np.uint64(16)) | halves[1].astype(np.uint64)).tolist()


def chain(spins, q, periodic, J, h, T, n_sweeps, seed, sweep0=0, replica=0, record_every=0, block=4096):
    """n_sweeps heat-bath sweeps of a tiny lattice in plain Python arithmetic.  Returns (final int8 array, codes): the state_code
    after every record_every-th sweep (none if 0).  Equal to `sweep` bit for bit (tests/test_potts_cpu.py compares them)."""
    s0 = np.array(spins, dtype=np.int8)
    rows, cols = s0.shape
    n = rows * cols
    E, F = (a.tolist() for a in tables(q, J, h, T))
    nbs = _site_lists(rows, cols, periodic)
    of_colour = [[i for i in range(n) if ((i // cols + i % cols) & 1) == col] for col in (0, 1)]
    s = s0.ravel().tolist()
    powers = [int(q) ** i for i in range(n)]
    codes = []
    done = 0
    while done < n_sweeps:
        nb_sweeps = min(block, n_sweeps - done)
        U = _uniform_block(rows, cols, int(sweep0) + done, nb_sweeps, seed, replica)
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
    return np.array(s, np.int8).reshape(rows, cols), codes


def cluster_chain(spins, q, periodic, J, T, n_steps, seed, step0=0, replica=0, record_every=0, block=4096):
    """n_steps Swendsen-Wang steps of a tiny lattice in plain Python integers.  Returns (final int8 array, codes).  Equal to
    `cluster_sweep` bit for bit."""
    s0 = np.array(spins, dtype=np.int8)
    rows, cols = s0.shape
    n = rows * cols
    thr = threshold(J, T)
    bonds = []  # (site, neighbour, which of the site's two bond words)
    for r in range(rows):
        for c in range(cols):
            if c + 1 < cols or periodic:
                bonds.append((r * cols + c, r * cols + (c + 1) % cols, 0))
            if r + 1 < rows or periodic:
                bonds.append((r * cols + c, ((r + 1) % rows) * cols + c, 1))
    R = np.repeat(np.arange(rows), cols)
    Cc = np.tile(np.arange(cols), rows)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    s = s0.ravel().tolist()
    powers = [int(q) ** i for i in range(n)]
    codes = []
    done = 0
    while done < n_steps:
        nb = min(block, n_steps - done)
        t = (int(step0) + done + np.arange(nb, dtype=np.uint64))[:, None]
        Wb = np.stack(philox4x32_10((Cc >> 1)[None, :], R[None, :], t, TAG_SW_BOND | (int(replica) << 8), k0, k1))
        Wf = np.stack(philox4x32_10((Cc >> 2)[None, :], R[None, :], t, TAG_SW_FLIP | (int(replica) << 8), k0, k1))
        sel = np.arange(n)[None, :]
        steps = np.arange(nb)[:, None]
        u_bond = [Wb[(2 * (Cc & 1) + d)[None, :], steps, sel].tolist() for d in (0, 1)]
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
    return np.array(s, np.int8).reshape(rows, cols), codes

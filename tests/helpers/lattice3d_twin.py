"""NumPy twin of K8's heat-bath sweep of a 3-D lattice with quenched disorder (csrc/ising3d.hip), bit for bit, vectorised per colour.

Contract, for a (D, R, C) lattice of +-1 spins and float32 disorder J_right, J_down, J_layer, h, with
periodic = (p_z, p_r, p_c) (a bool means all three):
  colour of a site = (z + r + c) & 1; sweep t = half-sweep hs = 2 t (colour 0), then hs = 2 t + 1 (colour 1)
  f   = ((((((J_layer[z-1] s[z-1]) + J_layer[z] s[z+1]) + J_down[r-1] s[r-1]) + J_down[r] s[r+1]) + J_right[c-1] s[c-1])
        + J_right[c] s[c+1]) + h in float64, a neighbour missing on an open axis skipped (no +0.0)
  x   = 2 f / T,  p = sigmoid(x) clamped at +-20,  thr = floor(p 2^32 + 1/2);  the site becomes +1 iff u < thr
  u   = K1's 32-bit site uniform with the global row rho = z R + r in place of r:
        disorder_twin.site_uniforms(D * R, C, hs, seed, replica).reshape(D, R, C)
With D = 1 and p_z = False this is disorder_twin.sweep.
"""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("disorder_twin", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                             "disorder_twin.py"))
_dt = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_dt)
site_uniforms_2d = _dt.site_uniforms
thresholds = _dt.thresholds


def axes(periodic):
    """(p_z, p_r, p_c) from a bool or a triple."""
    if isinstance(periodic, (bool, np.bool_)):
        return (bool(periodic),) * 3
    p = tuple(bool(x) for x in periodic)
    assert len(p) == 3
    return p


def site_uniforms(shape, hs, seed, replica=0):
    """(D, R, C) uint32: every site's u in half-sweep hs."""
    D, R, C = shape
    return site_uniforms_2d(D * R, C, hs, seed, replica).reshape(D, R, C)


def colours(shape):
    D, R, C = shape
    return (np.arange(D)[:, None, None] + np.arange(R)[None, :, None] + np.arange(C)[None, None, :]) & 1


def as_disorder(shape, J_right, J_down, J_layer, h=None):
    """The fp32 arrays the device stores (h=None: zero field)."""
    jr, jd, jl = (np.ascontiguousarray(a, dtype=np.float32).reshape(shape) for a in (J_right, J_down, J_layer))
    hh = np.zeros(shape, np.float32) if h is None else np.ascontiguousarray(h, dtype=np.float32).reshape(shape)
    return jr, jd, jl, hh


def neighbour_sum(s, periodic, jr, jd, jl):
    """(f, any): the float64 sum of the neighbour terms in the contract's order (z-1, z+1, r-1, r+1, c-1, c+1, a missing
    one skipped) and whether the site has a neighbour at all."""
    shape = s.shape
    pz, pr, pc = axes(periodic)
    s = s.astype(np.float64)
    Jr, Jd, Jl = (a.astype(np.float64) for a in (jr, jd, jl))
    idx = np.indices(shape)
    full = np.ones(shape, bool)
    terms = []
    for axis, J, per in ((0, Jl, pz), (1, Jd, pr), (2, Jr, pc)):
        n = shape[axis]
        terms.append((full if per else idx[axis] > 0, np.roll(J, 1, axis=axis) * np.roll(s, 1, axis=axis)))   # J[i-1] s[i-1]
        terms.append((full if per else idx[axis] < n - 1, J * np.roll(s, -1, axis=axis)))                     # J[i] s[i+1]
    f = np.zeros(shape)
    anyt = np.zeros(shape, bool)
    for hm, t in terms:
        f = np.where(hm, np.where(anyt, f + t, t), f)
        anyt = anyt | hm
    return f, anyt


def local_field(s, periodic, jr, jd, jl, h):
    """float64 f of every site in the contract's order."""
    f, anyt = neighbour_sum(s, periodic, jr, jd, jl)
    H = h.astype(np.float64)
    return np.where(anyt, f + H, H)


def half_sweep(s, periodic, jr, jd, jl, hh, T, hs, colour, seed, replica=0, stats=None):
    """One colour's update in half-sweep hs; returns a new int8 array."""
    u = site_uniforms(s.shape, hs, seed, replica).astype(np.uint64)
    thr = thresholds(local_field(s, periodic, jr, jd, jl, hh), T)
    mine = colours(s.shape) == colour
    if stats is not None:
        d = np.abs(u.astype(np.float64) - thr.astype(np.float64))
        stats["near"] = stats.get("near", 0) + int(np.count_nonzero(mine & (d < 65536.0)))
        stats["sites"] = stats.get("sites", 0) + int(np.count_nonzero(mine))
    return np.where(mine, np.where(u < thr, 1, -1), s).astype(np.int8)


def sweep(spins, periodic, J_right, J_down, J_layer, h, T, n_sweeps, seed, sweep0=0, replica=0, stats=None):
    """n_sweeps sweeps; returns a new int8 array.  stats (a dict) collects, per half-sweep, the count of sites whose u lies
    within 2^-16 (in units of 2^32) of its threshold, under 'near' and 'sites'."""
    s = np.array(spins, dtype=np.int8)
    assert s.ndim == 3
    jr, jd, jl, hh = as_disorder(s.shape, J_right, J_down, J_layer, h)
    for k in range(int(n_sweeps)):
        for colour in (0, 1):
            s = half_sweep(s, periodic, jr, jd, jl, hh, T, 2 * (int(sweep0) + k) + colour, colour, seed, replica, stats)
    return s


def energy_terms(spins, periodic, J_right, J_down, J_layer, h=None):
    """(E, sum of |terms|): E = -sum_bonds J s s' - sum h s in float64; the bonds an open axis does not have are dropped."""
    s = np.asarray(spins, dtype=np.float64)
    jr, jd, jl, hh = as_disorder(s.shape, J_right, J_down, J_layer, h)
    pz, pr, pc = axes(periodic)
    e = np.sum(hh.astype(np.float64) * s)
    a = np.sum(np.abs(hh.astype(np.float64)))
    for axis, J, per in ((2, jr, pc), (1, jd, pr), (0, jl, pz)):
        t = J.astype(np.float64) * s * np.roll(s, -1, axis=axis)
        if not per:
            t = np.delete(t, -1, axis=axis)
        e += np.sum(t)
        a += np.sum(np.abs(t))
    return -e, a


def energy(spins, periodic, J_right, J_down, J_layer, h=None):
    return energy_terms(spins, periodic, J_right, J_down, J_layer, h)[0]


def overlap(a, b):
    """q = sum_i a_i b_i (int)."""
    return int(np.sum(np.asarray(a, dtype=np.int64) * np.asarray(b, dtype=np.int64)))


def uniform_disorder(shape, periodic, J, h=0.0):
    """Constant arrays (J, h); the last slice of an open axis's J is 0."""
    pz, pr, pc = axes(periodic)
    jr, jd, jl = (np.full(shape, J, np.float32) for _ in range(3))
    if not pc:
        jr[:, :, -1] = 0.0
    if not pr:
        jd[:, -1, :] = 0.0
    if not pz:
        jl[-1, :, :] = 0.0
    return jr, jd, jl, np.full(shape, h, np.float32)


def _tie_target(shape, T, seed, replica):
    """float64 f that puts each site's decision of sweep 0 on its threshold: T / 2 logit(u / 2^32), u the site's own uniform in
    its half-sweep (colour 0 from hs = 0, colour 1 from hs = 1)."""
    u0 = site_uniforms(shape, 0, seed, replica).astype(np.float64)
    u1 = site_uniforms(shape, 1, seed, replica).astype(np.float64)
    u = np.clip(np.where(colours(shape) == 0, u0, u1), 1.0, 4294967295.0) / 4294967296.0
    return 0.5 * float(T) * (np.log(u) - np.log1p(-u))


def tie_field(shape, T, seed, replica=0, spins=None, periodic=None, couplings=None):
    """fp32 h that puts every decision of sweep 0 on its threshold.  Without couplings (all J = 0): h = fp32(T / 2 logit(u)).
    With couplings = (J_right, J_down, J_layer), the start state `spins` and `periodic`: h = fp32(target - neighbour sum), the
    seven-term sum sits on the threshold; colour 1's neighbour sums are taken after the colour-0 half-sweep (they depend on its
    outcome, and colour 0's decisions do not depend on colour 1's h)."""
    target = _tie_target(shape, T, seed, replica)
    if couplings is None:
        return target.astype(np.float32)
    jr, jd, jl, _ = as_disorder(shape, *couplings)
    s = np.array(spins, dtype=np.int8).reshape(shape)
    col = colours(shape)
    h = np.zeros(shape, np.float32)
    f0, _ = neighbour_sum(s, periodic, jr, jd, jl)
    h = np.where(col == 0, (target - f0).astype(np.float32), h).astype(np.float32)
    s1 = half_sweep(s, periodic, jr, jd, jl, h, T, 0, 0, seed, replica)
    f1, _ = neighbour_sum(s1, periodic, jr, jd, jl)
    return np.where(col == 1, (target - f1).astype(np.float32), h).astype(np.float32)


# ---------------------------------------------------------------- exact enumeration of a small open lattice
def enumeration_disorder(shape, dseed):
    """Gaussian J_right, J_down, J_layer, h (drawn in that order from default_rng(dseed)) of an open lattice: the last slices of
    the three J set to 0."""
    rng = np.random.default_rng(dseed)
    jr, jd, jl, h = (rng.normal(size=shape).astype(np.float32) for _ in range(4))
    jr[:, :, -1] = 0.0
    jd[:, -1, :] = 0.0
    jl[-1, :, :] = 0.0
    return jr, jd, jl, h


def state_code(s):
    """The state as an integer: bit i = site i (row-major) is +1."""
    bits = (np.asarray(s).ravel() > 0).astype(np.int64)
    return int(np.sum(bits << np.arange(bits.size)))


def boltzmann_chi2(codes, shape, disorder, T):
    """chi^2 of the histogram of `codes` (state_code of each recorded state) against exp(-E / T) / Z of the open lattice: the
    states with expected count >= 5 one cell each, the rest pooled into one cell.  Returns (chi2, dof, p, pooled share of the
    probability)."""
    from scipy.stats import chi2 as chi2_dist
    n_sites = int(np.prod(shape))
    n_states = 1 << n_sites
    E = np.empty(n_states)
    for k in range(n_states):
        s = np.where((k >> np.arange(n_sites)) & 1, 1, -1).reshape(shape)
        E[k] = energy(s, False, *disorder)
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

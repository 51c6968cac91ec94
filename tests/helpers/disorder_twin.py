"""NumPy twin of K7's disordered heat-bath sweep (csrc/ising2d_disorder.hip), bit for bit, vectorised per colour.

Contract, for a (rows, cols) lattice of +-1 spins and float32 disorder J_right, J_down, h:
  f   = (((J_down[r-1,c] s_up + J_down[r,c] s_down) + J_right[r,c-1] s_left) + J_right[r,c] s_right) + h[r,c] in float64,
        a neighbour missing on an open lattice skipped (no +0.0)
  x   = 2 f / T,  p = sigmoid(x) clamped at +-20,  thr = floor(p 2^32 + 1/2)
  the site becomes +1 iff u < thr, u = K1's 32-bit site uniform in half-sweep hs = 2 sweep + colour (colour 0 = (r + c) even):
        hi16 = half (m & 1) of word m >> 1 of Philox(c >> 4, r, hs, TAG_ISING_HI | replica << 8) with its top bit flipped,
        lo16 = the same half of the TAG_ISING_LO block, m = (c >> 1) & 7.  (The device draws lo16 only on a tie of the top 16
        bits; with the full u the comparison has the same outcome.)
"""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("cluster_twin", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                            "cluster_twin.py"))
_ct = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_ct)
philox4x32_10 = _ct.philox4x32_10

TAG_ISING_HI = 0
TAG_ISING_LO = 1


def site_uniforms(rows, cols, hs, seed, replica=0):
    """(rows, cols) uint32: every site's u in half-sweep hs (as oracle.ising2d_site_uniforms)."""
    noct = (cols + 15) >> 4
    R = np.arange(rows, dtype=np.uint64)[:, None]
    O = np.arange(noct, dtype=np.uint64)[None, :]
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    c = np.arange(cols)
    m = (c >> 1) & 7
    o = c >> 4
    word = m >> 1
    shift = (16 * (m & 1)).astype(np.uint32)
    out = []
    for tag in (TAG_ISING_HI, TAG_ISING_LO):
        W = np.stack(philox4x32_10(O, R, int(hs), tag | (int(replica) << 8), k0, k1))  # (4, rows, noct)
        out.append((W[word[None, :], np.arange(rows)[:, None], o[None, :]] >> shift[None, :]) & np.uint32(0xFFFF))
    hi = out[0] ^ np.uint32(0x8000)
    return ((hi.astype(np.uint64) << np.uint64(16)) | out[1].astype(np.uint64)).astype(np.uint32)


def as_disorder(rows, cols, J_right, J_down, h=None):
    """The fp32 arrays the device stores (h=None: zero field)."""
    jr = np.ascontiguousarray(J_right, dtype=np.float32).reshape(rows, cols)
    jd = np.ascontiguousarray(J_down, dtype=np.float32).reshape(rows, cols)
    hh = np.zeros((rows, cols), np.float32) if h is None else np.ascontiguousarray(h, dtype=np.float32).reshape(rows, cols)
    return jr, jd, hh


def local_field(s, periodic, jr, jd, h):
    """float64 f of every site in the contract's order (neighbours up, down, left, right, then h)."""
    rows, cols = s.shape
    s = s.astype(np.float64)
    Jr, Jd, H = (a.astype(np.float64) for a in (jr, jd, h))
    r = np.arange(rows)[:, None]
    c = np.arange(cols)[None, :]
    full = np.ones((rows, cols), bool)
    if periodic:
        has = (full, full, full, full)
    else:
        has = (np.broadcast_to(r > 0, (rows, cols)), np.broadcast_to(r < rows - 1, (rows, cols)),
               np.broadcast_to(c > 0, (rows, cols)), np.broadcast_to(c < cols - 1, (rows, cols)))
    terms = (np.roll(Jd, 1, axis=0) * np.roll(s, 1, axis=0),    # up:    J_down[r-1, c] s[r-1, c]
             Jd * np.roll(s, -1, axis=0),                        # down:  J_down[r, c]   s[r+1, c]
             np.roll(Jr, 1, axis=1) * np.roll(s, 1, axis=1),    # left:  J_right[r, c-1] s[r, c-1]
             Jr * np.roll(s, -1, axis=1))                        # right: J_right[r, c]  s[r, c+1]
    f = np.zeros((rows, cols))
    anyt = np.zeros((rows, cols), bool)
    for hm, t in zip(has, terms):
        f = np.where(hm, np.where(anyt, f + t, t), f)
        anyt = anyt | hm
    return np.where(anyt, f + H, H)


def thresholds(f, T):
    """uint64 thr = floor(sigmoid(2 f / T) 2^32 + 1/2), sigmoid clamped at +-20."""
    x = (2.0 * f) / float(T)
    with np.errstate(over="ignore"):
        p = np.where(x > 20.0, 1.0, np.where(x < -20.0, 0.0, 1.0 / (1.0 + np.exp(-np.clip(x, -30.0, 30.0)))))
    return np.floor(p * 4294967296.0 + 0.5).astype(np.uint64)


def sweep(spins, periodic, J_right, J_down, h, T, n_sweeps, seed, sweep0=0, replica=0, stats=None):
    """n_sweeps disordered sweeps; returns a new int8 array.  stats (a dict) collects, per half-sweep, the count of sites
    whose u lies within 2^-16 (in units of 2^32) of its threshold, under 'near' and 'sites'."""
    s = np.array(spins, dtype=np.int8)
    rows, cols = s.shape
    jr, jd, hh = as_disorder(rows, cols, J_right, J_down, h)
    colour_of = (np.arange(rows)[:, None] + np.arange(cols)[None, :]) & 1
    for k in range(int(n_sweeps)):
        for colour in (0, 1):
            hs = 2 * (int(sweep0) + k) + colour
            u = site_uniforms(rows, cols, hs, seed, replica).astype(np.uint64)
            thr = thresholds(local_field(s, periodic, jr, jd, hh), T)
            mine = colour_of == colour
            if stats is not None:
                d = np.abs(u.astype(np.float64) - thr.astype(np.float64))
                stats["near"] = stats.get("near", 0) + int(np.count_nonzero(mine & (d < 65536.0)))
                stats["sites"] = stats.get("sites", 0) + int(np.count_nonzero(mine))
            s = np.where(mine, np.where(u < thr, 1, -1), s).astype(np.int8)
    return s


def energy(spins, periodic, J_right, J_down, h=None):
    """E = -sum_bonds J s s' - sum h s in float64 (an open lattice's last column / row of J are 0 and add nothing)."""
    rows, cols = np.shape(spins)
    jr, jd, hh = as_disorder(rows, cols, J_right, J_down, h)
    s = np.asarray(spins, dtype=np.float64)
    e = np.sum(jr.astype(np.float64) * s * np.roll(s, -1, axis=1)) + np.sum(jd.astype(np.float64) * s * np.roll(s, -1, axis=0))
    if not periodic:  # the wrap terms carry J = 0 by contract; drop them anyway
        e = np.sum(jr[:, :-1].astype(np.float64) * s[:, :-1] * s[:, 1:]) + np.sum(jd[:-1].astype(np.float64) * s[:-1] * s[1:])
    return -(e + np.sum(hh.astype(np.float64) * s))


def overlap(a, b):
    """q = sum_i a_i b_i (int)."""
    return int(np.sum(np.asarray(a, dtype=np.int64) * np.asarray(b, dtype=np.int64)))


def uniform_disorder(rows, cols, periodic, J, h=0.0):
    """Constant arrays (J, h); an open lattice's last column of J_right and last row of J_down are 0."""
    jr = np.full((rows, cols), J, np.float32)
    jd = np.full((rows, cols), J, np.float32)
    if not periodic:
        jr[:, -1] = 0.0
        jd[-1, :] = 0.0
    return jr, jd, np.full((rows, cols), h, np.float32)


def tie_field(rows, cols, T, seed, replica=0):
    """h[r, c] = fp32(T / 2 logit(u / 2^32)) from each site's own uniform in its half-sweep of sweep 0 (colour 0 from hs = 0,
    colour 1 from hs = 1): with J = 0 every decision of sweep 0 sits on its threshold."""
    u0 = site_uniforms(rows, cols, 0, seed, replica).astype(np.float64)
    u1 = site_uniforms(rows, cols, 1, seed, replica).astype(np.float64)
    colour_of = (np.arange(rows)[:, None] + np.arange(cols)[None, :]) & 1
    u = np.clip(np.where(colour_of == 0, u0, u1), 1.0, 4294967295.0) / 4294967296.0
    return (0.5 * float(T) * (np.log(u) - np.log1p(-u))).astype(np.float32)

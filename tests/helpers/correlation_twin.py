"""NumPy twin of the axis profiles and k_min Fourier modes (csrc/corr_dev.h), bit for bit, and the exact reference of chi(k_min).

Contract ("Correlation length"), for a site field f = s (one lattice) or s^a s^b (two of one shape):
  profile of axis d: P_d[x] = the int64 sum of f over all sites whose coordinate on axis d is x (exact, any summation order)
  tables of a periodic axis of length L, made on the host: cos(2 pi x / L), sin(2 pi x / L) in float64, x = 0 .. L - 1, with the
        angle computed as 2.0 * pi * x / L (left to right)
  mode F_d = sum_x P_d[x] (cos_d[x] + i sin_d[x]), real and imaginary part each summed in this fixed order:
        term[x] = float64(P_d[x]) * table[x], rounded (no fused multiply-add);
        partial[t], t = 0 .. 255, starts at 0.0 and adds term[t], term[t + 256], ... in ascending order;
        the 64 partials of each group g = t // 64 fold by halves: for off = 32, 16, 8, 4, 2, 1: p[l] = p[l] + p[l + off], l < off;
        F = (p_0[0] + p_1[0]) + (p_2[0] + p_3[0])
  an open axis has a profile and no mode (NaN here)
  xi_d = sqrt(<f_tot^2> / <|F_d|^2> - 1) / (2 sin(pi / L_d)), NaN where the radicand is negative
"""
import importlib.util
import os

import numpy as np


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


lattice3d_twin = _load("lattice3d_twin")
disorder_twin = _load("disorder_twin")
enumeration_disorder = lattice3d_twin.enumeration_disorder


def profiles(a, b=None):
    """Tuple of int64 arrays, one per axis of `a` (2-D or 3-D +-1 spins): the sums of a (of a * b) over all other axes."""
    f = np.asarray(a, dtype=np.int64)
    if b is not None:
        b = np.asarray(b, dtype=np.int64)
        assert b.shape == f.shape
        f = f * b
    out = []
    for d in range(f.ndim):
        P = np.zeros(f.shape[d], np.int64)
        for x in range(f.shape[d]):  # site by site along the axis: the plain definition
            P[x] = int(np.take(f, x, axis=d).sum(dtype=np.int64))
        out.append(P)
    return tuple(out)


def tables(L):
    """(cos, sin) float64 tables of an axis of length L."""
    x = np.arange(int(L), dtype=np.float64)
    ang = 2.0 * np.pi * x / float(L)
    return np.cos(ang), np.sin(ang)


def ordered_sum(terms):
    """The fixed-order float64 sum of the contract."""
    terms = np.asarray(terms, dtype=np.float64)
    partial = np.zeros(256, np.float64)
    for t in range(min(256, terms.size)):
        e = np.float64(0.0)
        for x in range(t, terms.size, 256):
            e = e + terms[x]
        partial[t] = e
    p = partial.reshape(4, 64).copy()
    for off in (32, 16, 8, 4, 2, 1):
        for l in range(off):
            p[:, l] = p[:, l] + p[:, l + off]
    return float((p[0, 0] + p[1, 0]) + (p[2, 0] + p[3, 0]))


def modes(profs, periodic):
    """complex128 array, one entry per axis: F_d of a periodic axis, NaN + NaN j of an open one.  `periodic`: a bool (all axes) or a
    flag per axis."""
    n = len(profs)
    per = (bool(periodic),) * n if isinstance(periodic, (bool, np.bool_)) else tuple(bool(p) for p in periodic)
    assert len(per) == n
    out = np.full(n, complex(np.nan, np.nan), dtype=np.complex128)
    for d in range(n):
        if per[d]:
            P = np.asarray(profs[d], dtype=np.int64).astype(np.float64)
            c, s = tables(P.size)
            out[d] = complex(ordered_sum(P * c), ordered_sum(P * s))
    return out


def xi(f2, F2, L):
    """xi of one axis of length L from <f_tot^2> and <|F|^2> (scalars or arrays); NaN where the radicand is negative."""
    f2, F2 = np.asarray(f2, dtype=np.float64), np.asarray(F2, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rad = f2 / F2 - 1.0
        root = np.sqrt(np.where(rad >= 0, rad, np.nan))
    return root / (2.0 * np.sin(np.pi / float(L)))


def _as_3d(shape, periodic, disorder):
    """A 2-D problem (rows, cols), disorder (J_right, J_down, h) as the one-layer 3-D problem."""
    if len(shape) == 3:
        per = lattice3d_twin.axes(periodic)
        return tuple(shape), per, tuple(disorder), 0
    R, C = shape
    per = (bool(periodic),) * 2 if isinstance(periodic, (bool, np.bool_)) else tuple(bool(p) for p in periodic)
    jr, jd, h = disorder
    z = np.zeros((1, R, C), np.float32)
    h3 = None if h is None else np.asarray(h, np.float32).reshape(1, R, C)
    return (1, R, C), (False,) + per, (np.asarray(jr, np.float32).reshape(1, R, C), np.asarray(jd, np.float32).reshape(1, R, C), z, h3), 1


def exact_spin_correlations(shape, periodic, disorder, T):
    """<s_i s_j> at temperature T of E = -sum_bonds J s s' - sum h s by enumerating every state: (N, N) float64, sites row-major."""
    shape, per, (jr, jd, jl, h), _ = _as_3d(shape, periodic, disorder)
    D, R, C = shape
    pz, pr, pc = per
    N = D * R * C
    assert N <= 20, "full enumeration"
    idx = np.arange(2 ** N, dtype=np.int64)
    S = np.empty((2 ** N, N), np.int8)
    for n in range(N):
        S[:, n] = 1 - 2 * ((idx >> n) & 1)
    site = lambda z, r, c: (z * R + r) * C + c  # noqa: E731
    E = np.zeros(2 ** N)
    for z in range(D):
        for r in range(R):
            for c in range(C):
                n = site(z, r, c)
                if pc or c + 1 < C:
                    E -= float(jr[z, r, c]) * (S[:, n] * S[:, site(z, r, (c + 1) % C)])
                if pr or r + 1 < R:
                    E -= float(jd[z, r, c]) * (S[:, n] * S[:, site(z, (r + 1) % R, c)])
                if pz or z + 1 < D:
                    E -= float(jl[z, r, c]) * (S[:, n] * S[:, site((z + 1) % D, r, c)])
                if h is not None:
                    E -= float(h[z, r, c]) * S[:, n]
    w = np.exp(-(E - E.min()) / float(T))
    w /= w.sum()
    Cm = np.zeros((N, N))
    for lo in range(0, 2 ** N, 1 << 16):
        Sb = S[lo:lo + (1 << 16)].astype(np.float64)
        Cm += Sb.T @ (Sb * w[lo:lo + (1 << 16), None])
    return Cm


def exact_chi_k(shape, periodic, disorder, T):
    """<|F_d|^2> of the overlap field q_i = s^a_i s^b_i of two independent replicas at temperature T, per axis of `shape` (NaN on an
    open axis): sum_{i,j} cos(k_d (x_i - x_j)) <s_i s_j>_T^2 with k_d = 2 pi / L_d and x the coordinate on axis d.  `disorder`:
    (J_right, J_down, J_layer, h or None) for a 3-D shape, (J_right, J_down, h or None) for a 2-D one."""
    shape3, per3, _, skip = _as_3d(shape, periodic, disorder)
    Cm = exact_spin_correlations(shape, periodic, disorder, T)
    coords = np.indices(shape3).reshape(3, -1)
    out = []
    for d in range(skip, 3):
        if not per3[d]:
            out.append(np.nan)
            continue
        x = coords[d].astype(np.float64)
        k = 2.0 * np.pi / shape3[d]
        out.append(float(np.sum(np.cos(k * (x[:, None] - x[None, :])) * Cm ** 2)))
    return np.array(out)

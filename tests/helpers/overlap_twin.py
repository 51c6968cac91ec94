"""NumPy twin of the link overlap (csrc/link_dev.h) and of the pairing and family rule of a population's walker pairs.

Contract ("Overlaps of walker pairs"), for two +-1 spin arrays a, b of one shape (2-D or 3-D):
  p_i = a_i b_i;  L = sum over bonds (i, j) of p_i p_j, an exact integer;  N_b = the number of bonds;  q_l = L / N_b
  bonds: those of the lattice's energy (lattice3d_twin.energy_terms): every site's bond to its successor on each axis, the last one
        of an open axis dropped, the wrap bond of a periodic axis kept.  A periodic axis of length 1 bonds every site to itself and one
        of length 2 bonds each pair twice, as the energy does.
  a 2-D lattice is the one-layer 3-D lattice with an open layer axis
  population of R walkers: pair i = (walker i, walker i + P), i < P = R // 2 (an odd R leaves the last walker out)
  families: walker i of the start founds family i; a step's `parent` row maps every walker to the walker it copies (itself if it
        survives): fam <- fam[parent].  A pair counts (is "valid") at a step iff its two walkers are of different families there.
"""
import numpy as np


def axes(shape, periodic):
    """One flag per axis of `shape` from a bool or a sequence."""
    n = len(shape)
    per = (bool(periodic),) * n if isinstance(periodic, (bool, np.bool_)) else tuple(bool(p) for p in periodic)
    assert len(per) == n
    return per


def bond_count(shape, periodic):
    """N_b, bond by bond."""
    per = axes(shape, periodic)
    n = 0
    for d, (L, p) in enumerate(zip(shape, per)):
        others = int(np.prod(shape)) // L
        n += others * (L if p else L - 1)
    return n


def link_overlap(a, b, periodic):
    """(L, N_b) of the two spin arrays: axis by axis, every site times its successor, then the wrap bond of a periodic axis (the
    last site times the first).  The products stay +-1, so int8 holds them; the sums are int64."""
    a, b = np.asarray(a, dtype=np.int8), np.asarray(b, dtype=np.int8)
    assert a.shape == b.shape and np.all(np.abs(a) == 1) and np.all(np.abs(b) == 1)
    p = a * b
    per = axes(p.shape, periodic)
    L = nb = 0
    for d in range(p.ndim):
        n = p.shape[d]
        lo = [slice(None)] * p.ndim
        hi = [slice(None)] * p.ndim
        lo[d], hi[d] = slice(0, n - 1), slice(1, n)
        t = p[tuple(lo)] * p[tuple(hi)]
        L += int(t.sum(dtype=np.int64))
        nb += t.size
        if per[d]:
            t = np.take(p, n - 1, axis=d) * np.take(p, 0, axis=d)
            L += int(t.sum(dtype=np.int64))
            nb += t.size
    return L, nb


def degree(shape, periodic, site):
    """Bonds that end at `site` (a self-bond of a periodic axis of length 1 does not change when the site flips: not counted; the
    double bond of a periodic axis of length 2 counts twice)."""
    per = axes(shape, periodic)
    deg = 0
    for d, (n, p) in enumerate(zip(shape, per)):
        if n == 1:
            continue
        if p:
            deg += 2
        else:
            deg += (site[d] > 0) + (site[d] + 1 < n)
    return deg


def pairs(R):
    """[(i, i + P)] for i < P = R // 2."""
    P = R // 2
    return [(i, i + P) for i in range(P)]


def pair_mask(parent):
    """bool (n_steps + 1, P): row k, pair i: the two walkers are of different families after k steps (row 0: the start)."""
    parent = np.asarray(parent)
    n, R = parent.shape
    fam = list(range(R))
    rows = [[fam[i] != fam[j] for i, j in pairs(R)]]
    for k in range(n):
        fam = [fam[int(parent[k, i])] for i in range(R)]
        rows.append([fam[i] != fam[j] for i, j in pairs(R)])
    return np.array(rows, dtype=bool).reshape(n + 1, R // 2)


def pair_rows(planes, periodic):
    """(q, L) int64 arrays over the pairs of the stacked planes (R, *shape): q = sum a b, L = the link overlap."""
    planes = np.asarray(planes)
    q, L = [], []
    for i, j in pairs(planes.shape[0]):
        q.append(int(np.sum(planes[i].astype(np.int64) * planes[j].astype(np.int64))))
        L.append(link_overlap(planes[i], planes[j], periodic)[0])
    return np.array(q, np.int64), np.array(L, np.int64)

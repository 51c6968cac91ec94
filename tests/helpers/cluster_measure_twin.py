"""Python-integer twin of the cluster-size records (include/tsu_hip_cluster_measure.h): one row of 8 words per Swendsen-Wang step
from the roots the step twins return (cluster_twin.labels, cluster3d_twin.labels, cluster_field_twin.labels).

A row: n_clusters, largest, sum |C|^2, sum M_C^2, sum M_C^4 (low word, high word), n_frozen, m_frozen; M_C = sum of the spins of
cluster C; the free clusters are the components that do not reach the ghost.  The spins are those BEFORE the step's flips (the row
does not change under them).  Everything is a Python int; `words` folds a row into the 8 int64 words the device writes.
"""
import importlib.util
import os

import numpy as np


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


twin2 = _load("cluster_twin")
twin3 = _load("cluster3d_twin")
twinf = _load("cluster_field_twin")

FIELDS = ("n_clusters", "largest", "sum_size2", "sum_m2", "sum_m4", "n_frozen", "m_frozen")


def record(roots, spins, frozen=None):
    """The row of one step as a dict of Python ints.  roots: per site, its component's root (any array shape); a root of -1, or
    frozen[site] true (the convention of cluster_field_twin.labels), puts the site into n_frozen / m_frozen."""
    r = np.asarray(roots, dtype=np.int64).ravel()
    s = np.asarray(spins, dtype=np.int64).ravel()
    fz = r < 0
    if frozen is not None:
        fz = fz | np.asarray(frozen, dtype=bool).ravel()
    out = dict.fromkeys(FIELDS, 0)
    out["n_frozen"] = int(fz.sum())
    out["m_frozen"] = int(s[fz].sum())
    size, mag = {}, {}
    for root, spin in zip(r[~fz].tolist(), s[~fz].tolist()):
        size[root] = size.get(root, 0) + 1
        mag[root] = mag.get(root, 0) + spin
    out["n_clusters"] = len(size)
    out["largest"] = max(size.values(), default=0)
    out["sum_size2"] = sum(v * v for v in size.values())
    out["sum_m2"] = sum(v * v for v in mag.values())
    out["sum_m4"] = sum(v ** 4 for v in mag.values())
    return out


def words(rec):
    """The 8 int64 words of a row (sum_m4 split into its unsigned low and high words, each read back as int64)."""
    lo, hi = rec["sum_m4"] & (2 ** 64 - 1), rec["sum_m4"] >> 64
    assert hi < 2 ** 64
    w = [rec["n_clusters"], rec["largest"], rec["sum_size2"], rec["sum_m2"], lo, hi, rec["n_frozen"], rec["m_frozen"]]
    return [v - 2 ** 64 if v >= 2 ** 63 else v for v in w]


def columns(recs):
    """A list of rows -> the dict of per-step arrays that cluster_record() returns (sum_m4 an object array of Python ints)."""
    out = {k: np.array([r[k] for r in recs], dtype=object if k == "sum_m4" else np.int64) for k in FIELDS}
    if not recs:
        out["sum_m4"] = np.empty(0, object)
    return out


def sweep_2d(spins, periodic, J, T, n_steps, seed, step0=0, replica=0):
    """n_steps steps of cluster_twin; (spins after, list of rows)."""
    s, recs = np.asarray(spins, dtype=np.int8), []
    for k in range(int(n_steps)):
        roots, _, _ = twin2.labels(s, periodic, J, T, seed, int(step0) + k, replica)
        recs.append(record(roots, s))
        s = twin2.step(s, periodic, J, T, seed, int(step0) + k, replica)
    return s, recs


def sweep_3d(spins, periodic, J_right, J_down, J_layer, T, n_steps, seed, step0=0, replica=0):
    """n_steps zero-field steps of cluster3d_twin; (spins after, list of rows)."""
    s, recs = np.asarray(spins, dtype=np.int8), []
    for k in range(int(n_steps)):
        roots, _ = twin3.labels(s, periodic, J_right, J_down, J_layer, T, seed, int(step0) + k, replica)
        recs.append(record(roots, s))
        s = twin3.step(s, periodic, J_right, J_down, J_layer, T, seed, int(step0) + k, replica)
    return s, recs


def sweep_field(spins, periodic, J_right, J_down, J_layer, h, T, n_steps, seed, step0=0, replica=0):
    """n_steps ghost-spin steps of cluster_field_twin; (spins after, list of rows)."""
    s, recs = np.asarray(spins, dtype=np.int8), []
    for k in range(int(n_steps)):
        roots, frozen, _, _ = twinf.labels(s, periodic, J_right, J_down, J_layer, h, T, seed, int(step0) + k, replica)
        recs.append(record(roots, s, frozen))
        s = twinf.step(s, periodic, J_right, J_down, J_layer, h, T, seed, int(step0) + k, replica)
    return s, recs

"""NumPy twin of K11, the multicanonical Potts walkers (csrc/potts_muca.hip, include/tsu_hip_potts_muca.h), bit for bit.

State: (W, D, R, C) int8 colours 0 .. q - 1, W independent walkers of one lattice; periodic = (p_z, p_r, p_c) (a bool means all
three).  n_eq counts the bonds whose ends agree; a periodic axis of length 2 counts its double bond twice, one of length 1 has none.
Any side >= 1, odd periodic sides included.  Site index i = (z R + r) C + c.

Sweep t = sweep0 + k (mod 2^32) of walker w visits the sites in index order:
  words  sites i and i ^ 1 share Philox(i >> 1, w, t, TAG_POTTS_MUCA | replica << 8), key = seed; word 2 (i & 1) is the proposal
         word P, word 2 (i & 1) + 1 the acceptance uniform u
  c'     = (c + 1 + ((P (q - 1)) >> 32)) mod q
  delta  = n_{c'} - n_c over the existing neighbours (a double neighbour twice)
  accept iff u < thr[n][delta], thr = 2^32 when lnW[n + delta] >= lnW[n], else floor(exp(lnW[n + delta] - lnW[n]) 2^32): math.exp
After every sweep every walker adds H[n] += 1, S1[n] += N_max, S2[n] += N_max^2 and moves its tunnel side (0 none, 1 low, 2 high).

`run` is vectorised over the walkers and sequential over the sites.
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


philox4x32_10 = _load("cluster_twin").philox4x32_10
TAG_POTTS_MUCA = 13
TWO32 = 4294967296.0
SIDE_NONE, SIDE_LOW, SIDE_HIGH = 0, 1, 2


def axes(periodic):
    if isinstance(periodic, (bool, np.bool_)):
        return (bool(periodic),) * 3
    p = tuple(bool(x) for x in periodic)
    assert len(p) == 3
    return p


def shape3(shape):
    """(D, R, C) from an int, (R, C) or (D, R, C)."""
    if np.isscalar(shape):
        return (1, int(shape), int(shape))
    s = tuple(int(v) for v in shape)
    return (1,) + s if len(s) == 2 else s


def neighbour_lists(shape, periodic):
    """Per site the indices of its existing neighbours, a double neighbour (periodic axis of length 2) twice."""
    D, R, C = shape
    per = axes(periodic)
    out = []
    for z in range(D):
        for r in range(R):
            for c in range(C):
                nb = []
                for axis, d in ((2, -1), (2, 1), (1, -1), (1, 1), (0, -1), (0, 1)):
                    p = [z, r, c]
                    p[axis] += d
                    if not 0 <= p[axis] < shape[axis]:
                        if not (per[axis] and shape[axis] >= 2):
                            continue
                        p[axis] %= shape[axis]
                    nb.append((p[0] * R + p[1]) * C + p[2])
                out.append(nb)
    return out


def geometry(shape, periodic):
    """(B, z_max): the bonds with their multiplicity; z_max = 4 for one layer with an open depth axis, else 6."""
    shape = shape3(shape)
    per = axes(periodic)
    B = sum(len(nb) for nb in neighbour_lists(shape, per)) // 2
    return B, (4 if shape[0] == 1 and not per[0] else 6)


def thresholds(B, z_max, lnw):
    """(B + 1, 2 z_max + 1) uint64: thr[n][delta + z_max], 0 where n + delta lies outside 0 .. B."""
    lnw = [float(v) for v in lnw]
    assert len(lnw) == B + 1
    out = np.zeros((B + 1, 2 * z_max + 1), np.uint64)
    for n in range(B + 1):
        for d in range(-z_max, z_max + 1):
            if 0 <= n + d <= B:
                out[n, d + z_max] = 2 ** 32 if lnw[n + d] >= lnw[n] else int(math.floor(math.exp(lnw[n + d] - lnw[n]) * TWO32))
    return out


def count(spins, q, periodic):
    """(n_eq (W,), N_c (W, q)) of (W, D, R, C) colours, recounted from the spins."""
    s = np.asarray(spins, dtype=np.int64)
    W = s.shape[0]
    flat = s.reshape(W, -1)
    n = np.zeros(W, np.int64)
    for i, nb in enumerate(neighbour_lists(s.shape[1:], periodic)):
        for j in nb:
            n += flat[:, i] == flat[:, j]
    assert not (n & 1).any()
    return n // 2, np.stack([(flat == c).sum(axis=1) for c in range(q)], axis=1)


def new_record(B):
    return {"H": np.zeros(B + 1, np.uint64), "S1": np.zeros(B + 1, np.uint64), "S2": np.zeros(B + 1, np.uint64)}


def run(spins, q, periodic, lnw, n_sweeps, seed, sweep0=0, replica=0, record=None, side=None, tunnels=None, bounds=None):
    """n_sweeps sweeps of every walker.  Returns a dict: spins (new int8 array), n, N (incremental), H, S1, S2 (added to `record`
    when one is passed), side, tunnels."""
    s = np.array(spins, dtype=np.int8)
    W = s.shape[0]
    shape = s.shape[1:]
    flat = s.reshape(W, -1).astype(np.int64)
    sites = flat.shape[1]
    B, zmax = geometry(shape, periodic)
    thr = thresholds(B, zmax, lnw)
    lists = neighbour_lists(shape, periodic)
    n, N = count(s, q, periodic)
    rec = new_record(B) if record is None else {k: np.array(record[k], dtype=np.uint64) for k in ("H", "S1", "S2")}
    side = np.zeros(W, np.int64) if side is None else np.array(side, dtype=np.int64)
    tunnels = np.zeros(W, np.uint32) if tunnels is None else np.array(tunnels, dtype=np.uint32)
    n_lo, n_hi = (0, max(B, 1)) if bounds is None else bounds
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    w = np.arange(W, dtype=np.uint64)
    pairs = np.arange((sites + 1) // 2, dtype=np.uint64)
    rows = np.arange(W)
    for k in range(int(n_sweeps)):
        t = (int(sweep0) + k) & 0xFFFFFFFF
        words = philox4x32_10(pairs[:, None], w[None, :], t, TAG_POTTS_MUCA | (int(replica) << 8), k0, k1)
        for i in range(sites):
            P = words[2 * (i & 1)][i >> 1].astype(np.uint64)
            u = words[2 * (i & 1) + 1][i >> 1].astype(np.uint64)
            cur = flat[:, i]
            cn = (cur + 1 + ((P * np.uint64(q - 1)) >> np.uint64(32)).astype(np.int64)) % q
            d = np.zeros(W, np.int64)
            for j in lists[i]:
                d += (flat[:, j] == cn).astype(np.int64) - (flat[:, j] == cur).astype(np.int64)
            acc = u < thr[n, d + zmax]
            old = cur[acc].copy()
            flat[acc, i] = cn[acc]
            n = n + np.where(acc, d, 0)
            np.add.at(N, (rows[acc], old), -1)
            np.add.at(N, (rows[acc], cn[acc]), 1)
        assert n.min() >= 0 and n.max() <= B
        nmax = N.max(axis=1).astype(np.uint64)
        np.add.at(rec["H"], n, np.uint64(1))
        np.add.at(rec["S1"], n, nmax)
        np.add.at(rec["S2"], n, nmax * nmax)
        low, high = n <= n_lo, (n >= n_hi) & ~(n <= n_lo)
        tunnels = tunnels + ((low & (side == SIDE_HIGH)) | (high & (side == SIDE_LOW))).astype(np.uint32)
        side = np.where(low, SIDE_LOW, np.where(high, SIDE_HIGH, side))
    out = {"spins": flat.astype(np.int8).reshape(s.shape), "n": n, "N": N, "side": side, "tunnels": tunnels}
    out.update(rec)
    return out


# ---------------------------------------------------------------- enumeration of tiny lattices
def enumerate_states(shape, q, periodic):
    """(n_eq, N_max) of all q^N states, state code = sum_i s_i q^i, as int64 arrays."""
    shape = shape3(shape)
    sites = int(np.prod(shape))
    k = np.arange(int(q) ** sites, dtype=np.int64)
    digits = np.stack([(k // int(q) ** i) % int(q) for i in range(sites)], axis=1)
    n = np.zeros(len(k), np.int64)
    for i, nb in enumerate(neighbour_lists(shape, periodic)):
        for j in nb:
            n += digits[:, i] == digits[:, j]
    nmax = np.max(np.stack([(digits == c).sum(axis=1) for c in range(q)]), axis=0)
    return n // 2, nmax


def codes(spins, q):
    flat = np.asarray(spins, dtype=np.int64).reshape(len(spins), -1)
    return (flat * (int(q) ** np.arange(flat.shape[1], dtype=np.int64))[None, :]).sum(axis=1)


def weight_chi2(state_codes, shape, q, periodic, lnw):
    """chi^2 of the histogram of `state_codes` against W(n_eq(s)) / sum over the q^N states: the states with expected count >= 5
    one cell each, the rest pooled into one.  Returns (chi2, dof, p, pooled share of the probability)."""
    from scipy.stats import chi2 as chi2_dist
    n, _ = enumerate_states(shape, q, periodic)
    lw = np.asarray(lnw, dtype=np.float64)[n]
    prob = np.exp(lw - lw.max())
    prob /= prob.sum()
    expected = len(state_codes) * prob
    counts = np.bincount(np.asarray(state_codes, dtype=np.int64), minlength=len(n)).astype(np.float64)
    big = expected >= 5.0
    obs = np.append(counts[big], counts[~big].sum())
    exp = np.append(expected[big], expected[~big].sum())
    keep = exp > 0
    chi2 = float(np.sum((obs[keep] - exp[keep]) ** 2 / exp[keep]))
    dof = int(np.count_nonzero(keep)) - 1
    return chi2, dof, float(chi2_dist.sf(chi2, dof)), float(prob[~big].sum())


# The chi^2 table of the contract: (shape, q, periodic, seed of ln W = 0.3 n + 0.7 normal, chain seed); 16384 walkers, 200 sweeps
# from the all-0 state
CHI2_WALKERS, CHI2_SWEEPS = 16384, 200
CHI2_CASES = [((1, 2, 3), 3, False, 11, 5000),
              ((1, 3, 3), 2, False, 12, 5001),
              ((1, 2, 2), 4, (False, True, True), 13, 5002),
              ((2, 2, 2), 2, False, 14, 5003),
              ((1, 1, 5), 3, (False, False, True), 15, 5004)]


def chi2_weights(shape, periodic, seed):
    B, _ = geometry(shape, periodic)
    return 0.3 * np.arange(B + 1) + 0.7 * np.random.default_rng(seed).normal(size=B + 1)


"""NumPy / Python-integer twin of population annealing (tsu_pa2d_* / tsu_pa3d_*, csrc/pop_dev.h, csrc/pop_host.h).

Contract ("Population annealing"), R walkers on one disorder, schedule beta[0] < .. < beta[K]:
  walker i: a K7 / K8 lattice with key seed + i, replica 0, the shared sweep counter, the start of the lattice's randomize(seed + i)
  step k = 1 .. K, db = beta[k] - beta[k - 1], k_abs = k - 1 (the steps taken before it):
    E_min = min E;  W_i = rint(exp(-(db (E_i - E_min))) 2^30);  S = sum W
    U = (x64 S) >> 64, x64 = (w1 << 32) | w0 of Philox(0, 0, k_abs, TAG_POP_RESAMPLE = 11), key = seed
    n_i = (R C_i + U) // S - (R C_{i-1} + U) // S, C the inclusive prefix sums of W
    parent[i] = i where n_i >= 1; the dead indices, ascending, take the extra copies in ascending order of their source
    plane i := plane parent[i], then theta sweeps of every walker at T = 1 / beta[k] with key seed + i
The house rule of tempering_twin.py: the device's energies are fed in.  So are the device's weights W: `check_step` asserts they are
within one unit of NumPy's exp, and everything downstream is recomputed from them in Python integers, so a last-bit difference
between the two exps cannot fork the chain.

The sweeps are lattice3d_twin's, restated with a leading walker axis (`sweep_batch`: one call sweeps all walkers, each with its
own key); a 2-D lattice is the one-layer case (depth 1, open z, J_layer = 0), which lattice3d_twin documents to be
disorder_twin.sweep.  tests/test_population_cpu.py holds the restatement to the two twins bit for bit.
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
initial_spins_3d = _load("tempering3d_twin").initial_spins

TAG_POP_RESAMPLE = 11
ONE = 1 << 30
_MASK = np.uint64(0xFFFFFFFF)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 with counters AND keys broadcast against each other; four uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) & _MASK for x in (c0, c1, c2, c3, k0, k1)])
    for _ in range(10):
        p0 = _M0 * c0
        p1 = _M1 * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1 = p1 & _MASK
        c3 = p0 & _MASK
        c0, c2 = n0, n2
        k0 = (k0 + _W0) & _MASK
        k1 = (k1 + _W1) & _MASK
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


# ---------------------------------------------------------------------------------------------------- the resampler (integers)
def weights(E, db):
    """(W as a list of Python ints, E_min) from float64 energies: NumPy's exp."""
    E = np.asarray(E, dtype=np.float64)
    e_min = float(E.min())
    w = np.exp(-(float(db) * (E - e_min)))
    return [int(x) for x in np.rint(w * float(ONE))], e_min


def offset(S, k_abs, seed):
    """U = mulhi64(x64, S)."""
    w = philox(0, 0, int(k_abs), TAG_POP_RESAMPLE, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    x64 = (int(w[1]) << 32) | int(w[0])
    return (x64 * int(S)) >> 64


def counts(W, U):
    """n_i of systematic resampling at fixed size R = len(W), in Python integers."""
    R, S = len(W), sum(int(x) for x in W)
    assert 0 <= U < S
    n, C, before = [], 0, U // S
    for x in W:
        C += int(x)
        upto = (R * C + U) // S
        n.append(upto - before)
        before = upto
    return n


def placement(n):
    """(parent, dead, extra): survivors stay; dead[j] (ascending) takes extra[j] (sources ascending, source g n_g - 1 times)."""
    dead = [i for i, x in enumerate(n) if x == 0]
    extra = [g for g, x in enumerate(n) for _ in range(x - 1)]
    assert len(dead) == len(extra)
    parent = list(range(len(n)))
    for d, g in zip(dead, extra):
        parent[d] = g
    return parent, dead, extra


def resample(W, k_abs, seed):
    """{S, U, n, parent} of a step from its integer weights."""
    S = sum(int(x) for x in W)
    U = offset(S, k_abs, seed)
    n = counts(W, U)
    return {"S": S, "U": U, "n": n, "parent": placement(n)[0]}


def check_step(E, W_dev, db, k_abs, seed, S_dev, U_dev, Emin_dev, parent_dev):
    """Checks (a) and (b) of one step: the device's W within one unit of NumPy's, then S, U, E_min and parent recomputed from the
    device's E and W equal the device's exactly.  Returns the parents."""
    W_np, e_min = weights(E, db)
    W_dev = [int(x) for x in W_dev]
    worst = max(abs(a - b) for a, b in zip(W_dev, W_np))
    assert worst <= 1, f"weights differ from rint(exp(..) 2^30) by {worst} units"
    assert float(Emin_dev) == e_min, (Emin_dev, e_min)
    want = resample(W_dev, k_abs, seed)
    assert int(S_dev) == want["S"] and int(U_dev) == want["U"], (S_dev, want["S"], U_dev, want["U"])
    got = np.asarray(parent_dev, dtype=np.int64)
    bad = np.flatnonzero(got != np.asarray(want["parent"]))
    assert bad.size == 0, f"parent differs at {bad[:8]} ({bad.size} walkers)"
    return got


# ---------------------------------------------------------------------------------------------------- sweeps of all walkers at once
def as_3d(spins, periodic, disorder):
    """(spins (B, D, R, C), (p_z, p_r, p_c), (jr, jd, jl, h)) of a batch of 2-D lattices (B, R, C) with (jr, jd, h), or of 3-D ones
    unchanged."""
    spins = np.asarray(spins, dtype=np.int8)
    if len(disorder) == 3:
        jr, jd, h = disorder
        shape = (1,) + spins.shape[1:]
        jr, jd, hh = disorder_twin.as_disorder(shape[1], shape[2], jr, jd, h)
        return (spins[:, None], (False, bool(periodic), bool(periodic)),
                (jr.reshape(shape), jd.reshape(shape), np.zeros(shape, np.float32), hh.reshape(shape)))
    return spins, lattice3d_twin.axes(periodic), lattice3d_twin.as_disorder(spins.shape[1:], *disorder)


def site_uniforms_batch(shape, hs, seeds):
    """(B, D, R, C) uint32: lattice3d_twin.site_uniforms for every key of `seeds`."""
    D, R, C = shape
    seeds = [int(s) for s in seeds]
    k0 = np.array([s & 0xFFFFFFFF for s in seeds], np.uint64)[:, None, None]
    k1 = np.array([(s >> 32) & 0xFFFFFFFF for s in seeds], np.uint64)[:, None, None]
    noct = (C + 15) >> 4
    rho = np.arange(D * R, dtype=np.uint64)[None, :, None]
    octet = np.arange(noct, dtype=np.uint64)[None, None, :]
    c = np.arange(C)
    m = (c >> 1) & 7
    halves = []
    for tag in (0, 1):  # TAG_ISING_HI, TAG_ISING_LO
        W = np.stack(philox(octet, rho, int(hs), tag, k0, k1))  # (4, B, D R, noct)
        halves.append((W[m >> 1, :, :, c >> 4] >> (16 * (m & 1)).astype(np.uint32)[:, None, None]) & np.uint32(0xFFFF))  # (C, B, D R)
    hi = halves[0] ^ np.uint32(0x8000)
    u = (hi.astype(np.uint64) << np.uint64(16)) | halves[1].astype(np.uint64)
    return np.moveaxis(u, 0, -1).reshape(len(seeds), D, R, C).astype(np.uint32)


def local_field_batch(s, per, jr, jd, jl, h):
    """lattice3d_twin.local_field with a leading walker axis: the same terms in the same order."""
    shape = s.shape[1:]
    s = s.astype(np.float64)
    idx = np.indices(shape)
    full = np.ones(shape, bool)
    terms = []
    for axis, J, p in ((0, jl, per[0]), (1, jd, per[1]), (2, jr, per[2])):
        J = J.astype(np.float64)
        n = shape[axis]
        terms.append((full if p else idx[axis] > 0, np.roll(J, 1, axis=axis)[None] * np.roll(s, 1, axis=axis + 1)))
        terms.append((full if p else idx[axis] < n - 1, J[None] * np.roll(s, -1, axis=axis + 1)))
    f = np.zeros(s.shape)
    anyt = np.zeros(shape, bool)
    for hm, t in terms:
        f = np.where(hm[None], np.where(anyt[None], f + t, t), f)
        anyt = anyt | hm
    H = h.astype(np.float64)[None]
    return np.where(anyt[None], f + H, H)


def sweep_batch(spins, periodic, disorder, T, n_sweeps, seeds, sweep0):
    """n_sweeps sweeps of every walker of the batch (2-D: (B, R, C) with disorder (jr, jd, h); 3-D: (B, D, R, C) with (jr, jd, jl,
    h)), walker b with key seeds[b], replica 0, sweep counters sweep0 ..; returns a new int8 array of the input's shape."""
    in_shape = np.shape(spins)
    s, per, (jr, jd, jl, hh) = as_3d(spins, periodic, disorder)
    s = np.array(s, dtype=np.int8)
    mine0 = lattice3d_twin.colours(s.shape[1:])
    for k in range(int(n_sweeps)):
        for colour in (0, 1):
            u = site_uniforms_batch(s.shape[1:], 2 * (int(sweep0) + k) + colour, seeds).astype(np.uint64)
            thr = lattice3d_twin.thresholds(local_field_batch(s, per, jr, jd, jl, hh), T)
            s = np.where((mine0 == colour)[None], np.where(u < thr, 1, -1), s).astype(np.int8)
    return s.reshape(in_shape)


def initial_spins(shape, seed, n_walkers):
    """(B, ...) int8: walker i's start, the lattice's randomize(seed + i) (2-D shapes are the one-layer case of the 3-D draw)."""
    shape3 = (1,) + tuple(shape) if len(shape) == 2 else tuple(shape)
    return np.stack(initial_spins_3d(shape3, seed, n_walkers)).reshape((n_walkers,) + tuple(shape))


def check_chain(betas, seed, theta, periodic, disorder, spins0, record, planes_after, step0=0, sweep0=0):
    """Checks (a)-(c) along a recorded chain.  `record`: the handle's history of the steps step0 + 1 .. step0 + n (E (n + 1, R), W,
    parent, S, U, E_min); `planes_after[j]`: all planes (R, ...) after step j of the record; spins0: the planes before its first
    step; sweep0: the sweep counter there.  Returns the fraction of walkers that died per step."""
    R = np.shape(spins0)[0]
    seeds = [int(seed) + i for i in range(R)]
    before = np.asarray(spins0)
    died = []
    for j in range(len(record["S"])):
        k = step0 + j + 1
        parent = check_step(record["E"][j], record["W"][j], betas[k] - betas[k - 1], k - 1, seed, record["S"][j], record["U"][j],
                            record["E_min"][j], record["parent"][j])
        died.append(float(np.mean(parent != np.arange(R))))
        want = sweep_batch(before[parent], periodic, disorder, 1.0 / betas[k], theta, seeds, sweep0 + j * theta)
        bad = np.flatnonzero((np.asarray(planes_after[j]) != want).reshape(R, -1).any(axis=1))
        assert bad.size == 0, f"step {k}: planes of walkers {bad[:8]} ({bad.size} in all) differ from spins_before[parent] swept"
        before = np.asarray(planes_after[j])
    return died

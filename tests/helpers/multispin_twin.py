"""NumPy twin of K9, the multispin-coded +-J glass (csrc/multispin.hip): 64 disorder samples per uint64 word.

Contract ("Multispin coding (K9)"): bit b of word-plane w is sample 64 w + b, a set bit is spin +1, a set
coupling bit is J = -1, pad bits carry J = +1.  Sample s of a plane with seed `seed` at temperature T takes the decisions of
lattice3d_twin.sweep(spins, periodic, J_right[s], J_down[s], J_layer[s], None, T, n, seed, sweep0), replica 0.

Two statements of the same thing live here: `reference_sweep`, the per-sample loop over lattice3d_twin (the yardstick), and
`bitsliced_sweep`, the update as the kernels do it on packed words (adder, count >= k*, lo16 only on a hi16 tie).
"""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("lattice3d_twin", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                              "lattice3d_twin.py"))
lat3 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lat3)

ALL = np.uint64(0xFFFFFFFFFFFFFFFF)
ZERO = np.uint64(0)


def pack(bits):
    """(S, ...) booleans -> (ceil(S / 64), ...) uint64; pad bits 0."""
    bits = np.asarray(bits, dtype=bool)
    S, shape = bits.shape[0], bits.shape[1:]
    W = (S + 63) // 64
    out = np.zeros((W,) + shape, np.uint64)
    for s in range(S):
        out[s // 64] |= bits[s].astype(np.uint64) << np.uint64(s % 64)
    return out


def unpack(words, n_samples):
    """(W, ...) uint64 -> (n_samples, ...) booleans."""
    words = np.asarray(words, dtype=np.uint64)
    return np.stack([((words[s // 64] >> np.uint64(s % 64)) & np.uint64(1)).astype(bool) for s in range(int(n_samples))])


def table(T):
    """The 13 thresholds of a slot: table[f + 6] = thr(f), f = -6 .. 6 (disorder_twin.thresholds)."""
    return lat3.thresholds(np.arange(-6, 7, dtype=np.float64), T)


def reference_sweep(spins, periodic, couplings, T, n_sweeps, seed, sweep0=0):
    """spins (S, D, R, C) int8, couplings three (S, D, R, C) arrays: every sample through lattice3d_twin.sweep."""
    return np.stack([lat3.sweep(spins[s], periodic, couplings[0][s], couplings[1][s], couplings[2][s], None, T, n_sweeps, seed, sweep0)
                     for s in range(spins.shape[0])])


def reference_energy(spins, periodic, couplings):
    return np.array([lat3.energy(spins[s], periodic, couplings[0][s], couplings[1][s], couplings[2][s]) for s in range(spins.shape[0])])


def _split_uniforms(shape, hs, seed):
    """(hi16, lo16) of every site's uniform in half-sweep hs, replica 0."""
    u = lat3.site_uniforms(shape, hs, seed).astype(np.uint64)
    return u >> np.uint64(16), u & np.uint64(0xFFFF)


def neighbour_words(s, periodic, jr, jd, jl):
    """(x, n): the six words 'bond contributes +1' of every site (zero where the neighbour is missing) in the order z-1, z+1, r-1,
    r+1, c-1, c+1, and the number of neighbours present.  s, jr, jd, jl: (W, D, R, C) uint64."""
    shape = s.shape[1:]
    per = lat3.axes(periodic)
    idx = np.indices(shape)
    xs = []
    n = np.zeros(shape, np.int64)
    for axis, J in ((0, jl), (1, jd), (2, jr)):
        L = shape[axis]
        has_prev = np.ones(shape, bool) if per[axis] else idx[axis] > 0
        has_next = np.ones(shape, bool) if per[axis] else idx[axis] < L - 1
        prev = np.roll(s, 1, axis=axis + 1) ^ np.roll(J, 1, axis=axis + 1)
        nxt = np.roll(s, -1, axis=axis + 1) ^ J
        xs.append(np.where(has_prev[None], prev, ZERO))
        xs.append(np.where(has_next[None], nxt, ZERO))
        n += has_prev.astype(np.int64) + has_next.astype(np.int64)
    return xs, n


def adder(xs):
    """Three count planes (b0, b1, b2) of six one-bit words: count = b0 + 2 b1 + 4 b2."""
    a, b, c, d, e, f = xs
    s1, c1 = a ^ b ^ c, (a & b) | (c & (a ^ b))
    s2, c2 = d ^ e ^ f, (d & e) | (f & (d ^ e))
    c3 = s1 & s2
    return s1 ^ s2, c1 ^ c2 ^ c3, (c1 & c2) | (c3 & (c1 ^ c2))


def kstar(tab, n, u):
    """k* per site: the number of k in 0 .. n with u >= thr(2 k - n); also whether a candidate's top 16 bits equal u's."""
    ks = np.zeros(n.shape, np.int64)
    tie = np.zeros(n.shape, bool)
    for k in range(7):
        valid = k <= n
        t = tab[np.where(valid, 2 * k - n + 6, 12)]
        ks += (valid & (u >= t)).astype(np.int64)
        tie |= valid & ((t >> np.uint64(16)) == (u >> np.uint64(16)))
    return ks, tie


def at_least(b0, b1, b2, ks):
    """The word 'count >= k*': the carry out of count + (8 - k*) in three bits; k* = 0 is every sample."""
    d = 8 - ks
    d0, d1, d2 = (np.where((d >> i) & 1, ALL, ZERO)[None] for i in range(3))
    maj = lambda a, b, c: (a & b) | (c & (a ^ b))
    return np.where((ks == 0)[None], ALL, maj(b2, d2, maj(b1, d1, b0 & d0)))


def bitsliced_half_sweep(s, periodic, jr, jd, jl, tab, hs, colour, seed, stats=None):
    shape = s.shape[1:]
    hi, lo = _split_uniforms(shape, hs, seed)
    xs, n = neighbour_words(s, periodic, jr, jd, jl)
    b0, b1, b2 = adder(xs)
    u = hi << np.uint64(16)
    ks, tie = kstar(tab, n, u)
    mine = lat3.colours(shape) == colour
    if stats is not None:
        stats["ties"] = stats.get("ties", 0) + int(np.count_nonzero(tie & mine))
    ks_full, _ = kstar(tab, n, u | lo)  # the lo16 half enters only where hi16 ties
    ks = np.where(tie, ks_full, ks)
    return np.where(mine[None], at_least(b0, b1, b2, ks), s)


def bitsliced_sweep(s, periodic, jr, jd, jl, T, n_sweeps, seed, sweep0=0, stats=None):
    """n_sweeps sweeps of packed planes (W, D, R, C) with packed couplings, as the kernels take them."""
    s = np.array(s, dtype=np.uint64)
    tab = table(T)
    for k in range(int(n_sweeps)):
        for colour in (0, 1):
            s = bitsliced_half_sweep(s, periodic, jr, jd, jl, tab, 2 * (int(sweep0) + k) + colour, colour, seed, stats)
    return s


def sample_ties(spins, periodic, couplings, T, n_sweeps, seed, sweep0=0):
    """Per-sample count, with lattice3d_twin's own field and threshold, of the updates whose threshold shares its top 16 bits with
    the site's uniform: the decisions that need the lo16 block."""
    ties = 0
    s = np.array(spins, dtype=np.int8)
    for smp in range(s.shape[0]):
        x = s[smp]
        d = lat3.as_disorder(x.shape, couplings[0][smp], couplings[1][smp], couplings[2][smp])
        for k in range(int(n_sweeps)):
            for colour in (0, 1):
                hs = 2 * (int(sweep0) + k) + colour
                u = lat3.site_uniforms(x.shape, hs, seed).astype(np.uint64)
                thr = lat3.thresholds(lat3.local_field(x, periodic, *d), T)
                mine = lat3.colours(x.shape) == colour
                ties += int(np.count_nonzero(mine & ((thr >> np.uint64(16)) == (u >> np.uint64(16)))))
                x = lat3.half_sweep(x, periodic, *d, T, hs, colour, seed)
    return ties


def counters_add(planes, x):
    """Add the one-bit word array x into bit-sliced vertical counters (a list of planes, least significant first)."""
    out = []
    for p in planes:
        out.append(p ^ x)
        x = p & x
    assert not np.any(x), "vertical counter overflow"
    return out


def counters_values(planes):
    """(64,) + shape integers: counter b of every word position."""
    v = np.zeros((64,) + planes[0].shape, np.int64)
    for k, p in enumerate(planes):
        for b in range(64):
            v[b] += ((p >> np.uint64(b)) & np.uint64(1)).astype(np.int64) << k
    return v

"""NumPy twin of K9's axis profiles and k_min modes (tsu_msc_profiles / _modes, csrc/multispin_corr.hip).

Contract ("Correlation length of multispin-coded glasses (K9)").  Per slot t and sample s the site field is
f = a b, the slot's two replicas, or f = s with one; P_d[x] = the exact integer sum of f over the sites with coordinate x on axis d;
F_d = correlation_twin.modes of those profiles (NaN on an open axis).

Two statements of the profiles live here: `profiles`, which unpacks the planes and takes correlation_twin.profiles per sample (the
yardstick), and `packed_profiles`, the positional count as the kernel does it on packed words: x = a ^ b (or ~a) has a set bit
where f = -1; the n_x sites of a coordinate are cut into parts of at most 64 * 255 sites; lane l of 64 adds the words l, l + 64,
... of a part into 8 bit-sliced counter planes (at most 255 additions: no overflow); per counter plane k and bit b the number of
lanes with that bit set, times 2^k, goes to sample b's total; the part's share is its site count - 2 total.
"""
import importlib.util
import os

import numpy as np


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


msc = _load("multispin_twin")
corr = _load("correlation_twin")

LANES, ADDS, PLANES = 64, 255, 8


def spins_of(planes, S):
    """(R, A, W, D, Rr, C) uint64 -> int8 (R, A, S, D, Rr, C) spins."""
    planes = np.asarray(planes, dtype=np.uint64)
    R, A = planes.shape[:2]
    return np.stack([np.stack([np.where(msc.unpack(planes[t, a], S), 1, -1).astype(np.int8) for a in range(A)]) for t in range(R)])


def profiles(planes, S):
    """(P_z, P_r, P_c), int64 (R, S, L_d): correlation_twin.profiles of every sample's unpacked spins."""
    s = spins_of(planes, S)
    R, A = s.shape[:2]
    out = [np.zeros((R, S, n), np.int64) for n in s.shape[3:]]
    for t in range(R):
        for k in range(S):
            for d, P in enumerate(corr.profiles(s[t, 0, k], s[t, 1, k] if A == 2 else None)):
                out[d][t, k] = P
    return tuple(out)


def parts_of(n):
    """(parts, chunk) of a coordinate with n sites: the fewest parts of at most LANES * ADDS sites, of equal size but the last."""
    parts = (n + LANES * ADDS - 1) // (LANES * ADDS)
    return parts, (n + parts - 1) // parts


def _part_counts(words):
    """(64,) set bits per sample bit of a part's words (n,) uint64, n <= LANES * ADDS, by lanes, counter planes and ballots."""
    n = words.size
    assert n <= LANES * ADDS
    padded = np.zeros(LANES * ((n + LANES - 1) // LANES), np.uint64)
    padded[:n] = words
    steps = padded.reshape(-1, LANES)  # step k: lane l takes word l + 64 k (a lane past the end adds nothing)
    planes = [np.zeros(LANES, np.uint64) for _ in range(PLANES)]
    for x in steps:
        planes = msc.counters_add(planes, x)
    total = np.zeros(64, np.int64)
    for k, p in enumerate(planes):
        if not p.any():
            continue
        for b in range(64):
            ballot = (p >> np.uint64(b)) & np.uint64(1)
            total[b] += int(ballot.sum()) << k
    return total


def packed_profiles(planes, S, with_pad=False):
    """(P_z, P_r, P_c), int64 (R, S, L_d) (or (R, 64 W, L_d) with_pad), from the packed words alone."""
    planes = np.asarray(planes, dtype=np.uint64)
    R, A, W = planes.shape[:3]
    shape = planes.shape[3:]
    N = int(np.prod(shape))
    out = [np.zeros((R, 64 * W, n), np.int64) for n in shape]
    for t in range(R):
        for w in range(W):
            x = planes[t, 0, w] ^ planes[t, 1, w] if A == 2 else ~planes[t, 0, w]
            for d in range(3):
                n = N // shape[d]
                parts, chunk = parts_of(n)
                for c in range(shape[d]):
                    words = np.take(x, c, axis=d).ravel()  # j ascending: the other two coordinates, row-major
                    for p in range(parts):
                        part = words[p * chunk:(p + 1) * chunk]
                        out[d][t, 64 * w:64 * w + 64, c] += part.size - 2 * _part_counts(part)
    return tuple(o if with_pad else o[:, :S] for o in out)


def modes(profs, periodic):
    """complex128 (R, S, 3) from profiles (R, S, L_d): correlation_twin.modes of every (slot, sample)."""
    R, S = profs[0].shape[:2]
    out = np.zeros((R, S, 3), np.complex128)
    for t in range(R):
        for s in range(S):
            out[t, s] = corr.modes([P[t, s] for P in profs], periodic)
    return out


def same_bits(a, b):
    """complex arrays equal bit for bit: real and imaginary parts compared as uint64 (NaN payloads included)."""
    a, b = np.ascontiguousarray(a, dtype=np.complex128), np.ascontiguousarray(b, dtype=np.complex128)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())

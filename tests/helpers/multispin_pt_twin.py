"""NumPy twin of K9's tempering (tsu_msc_pt_*, csrc/multispin_pt.hip): the swap pass per sample and the exchange of configurations.

Contract ("Tempering of multispin-coded glasses (K9)").  Per replica a and sample s, independently, the pairs
i = 0 .. n_temps - 2 in order: E_x = the energy of the configuration now at slot i (an earlier swap of the pass may have moved it
there), E_y = that at slot i + 1, delta = (1.0 / T[i] - 1.0 / T[i + 1]) * (E_x - E_y), accept iff delta >= 0 or u < exp(delta),
u = tempering_twin.uniform53(i, round, TAG_PT_SWAP | a << 8, swap_seeds[s]).  An accepted pair exchanges the two configurations;
temperature and sweep seed stay with the slot.  Labels name the starting configurations; flags and trips follow tempering_twin.arrive.

The energies are fed in (the device's integers, exact), so only exp is left to differ between this file and the device.
"""
import importlib.util
import os

import numpy as np


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


pt = _load("tempering_twin")
msc = _load("multispin_twin")
TAG_PT_SWAP, NONE, BOTTOM, TOP = pt.TAG_PT_SWAP, pt.NONE, pt.BOTTOM, pt.TOP


class Book:
    """The book-keeping per (replica, sample): labels (A, S, R), flags and trips per label (A, S, R), attempts / accepts (A, S, R - 1)."""

    def __init__(self, A, S, R):
        self.A, self.S, self.R = A, S, R
        self.labels = np.tile(np.arange(R, dtype=np.int32), (A, S, 1))
        self.flags = np.full((A, S, R), NONE, np.int32)
        self.flags[:, :, 0] = BOTTOM
        self.trips = np.zeros((A, S, R), np.int64)
        self.attempts = np.zeros((A, S, R - 1), np.int64)
        self.accepts = np.zeros((A, S, R - 1), np.int64)
        self.rounds = 0


def swap_pass(book, T, E, swap_seeds):
    """One pass of round book.rounds.  E: (R, A, S) energies by slot.  Returns accept (R - 1, A, S) booleans; updates the book."""
    A, S, R = book.A, book.S, book.R
    T = [float(x) for x in T]
    accept = np.zeros((R - 1, A, S), bool)
    for a in range(A):
        for s in range(S):
            u = pt.uniform53(np.arange(R - 1), book.rounds, TAG_PT_SWAP | (a << 8), swap_seeds[s])
            lab, flags, trips = book.labels[a, s], book.flags[a, s], book.trips[a, s]
            ex, cur = float(E[0, a, s]), int(lab[0])
            for i in range(R - 1):
                ey, nxt = float(E[i + 1, a, s]), int(lab[i + 1])
                delta = (1.0 / T[i] - 1.0 / T[i + 1]) * (ex - ey)
                book.attempts[a, s, i] += 1
                if delta >= 0 or u[i] < np.exp(delta):
                    book.accepts[a, s, i] += 1
                    accept[i, a, s] = True
                    lab[i] = nxt
                    pt.arrive(flags, trips, cur, i + 1, R)
                    pt.arrive(flags, trips, nxt, i, R)
                else:
                    lab[i] = cur
                    cur, ex = nxt, ey
            lab[R - 1] = cur
    book.rounds += 1
    return accept


def pack_masks(accept):
    """(R - 1, A, S) booleans -> (R - 1, A, W) uint64 mask words, pad bits 0."""
    n, A, S = accept.shape
    W = (S + 63) // 64
    m = np.zeros((n, A, W), np.uint64)
    for s in range(S):
        m[:, :, s // 64] |= accept[:, :, s].astype(np.uint64) << np.uint64(s % 64)
    return m


def exchange(planes, masks):
    """planes (R, A, W, ...) uint64, masks (R - 1, A, W): the pairs in order, d = (x ^ y) & m; x ^= d; y ^= d.  A new array."""
    x = np.array(planes, dtype=np.uint64)
    extra = (1,) * (x.ndim - 3)
    for i in range(x.shape[0] - 1):
        d = (x[i] ^ x[i + 1]) & masks[i].reshape(masks[i].shape + extra)
        x[i] ^= d
        x[i + 1] ^= d
    return x


def _bits(words, S):
    """(W, ...) uint64 -> (S,) counts of set bits per sample over all sites (msc.unpack(words, S) summed per sample; the bits are
    taken apart by bytes, so that thousands of samples cost no more than a few)."""
    words = np.ascontiguousarray(words, dtype="<u8")
    W = words.shape[0]
    if words.size == 0:  # an open axis of length 1 has no bond
        return np.zeros(S, np.int64)
    bits =np.unpackbits(words.reshape(W, -1).view(np.uint8).reshape(W, -1, 8), axis=-1, bitorder="little")  # (W, sites, 64)
    return bits.sum(axis=1, dtype=np.int64).reshape(W * 64)[:S]


def measure(planes, periodic, jr, jd, jl, S):
    """k9_measure's integers from packed planes (R, A, W, D, Rr, C) and packed couplings (W, D, Rr, C): unsat, sum (R, A, S) and,
    with two replicas, q and q_link (R, S), scaled like tsu_msc_measure's outputs; also the bond count."""
    planes = np.asarray(planes, dtype=np.uint64)
    R, A = planes.shape[:2]
    shape = planes.shape[3:]
    per = msc.lat3.axes(periodic)
    N = int(np.prod(shape))
    nb = sum(N if per[ax] else N // shape[ax] * (shape[ax] - 1) for ax in range(3))
    unsat, up = np.zeros((R, A, S), np.int64), np.zeros((R, A, S), np.int64)
    q, ql = np.zeros((R, S), np.int64), np.zeros((R, S), np.int64)
    for t in range(R):
        diff = []
        for a in range(A):
            x = planes[t, a]
            up[t, a] = _bits(x, S)
            d = []
            for axis, J in ((2, jr), (1, jd), (0, jl)):
                keep = [slice(None)] * 4
                if not per[axis]:
                    keep[axis + 1] = slice(0, shape[axis] - 1)  # an open axis lacks its last bond
                dx = x ^ np.roll(x, -1, axis=axis + 1)
                unsat[t, a] += _bits((dx ^ J)[tuple(keep)], S)
                d.append(dx[tuple(keep)])
            diff.append(d)
        if A == 2:
            q[t] = N - 2 * _bits(planes[t, 0] ^ planes[t, 1], S)
            ql[t] = nb - 2 * sum(_bits(da ^ db, S) for da, db in zip(*diff))
    return unsat, 2 * up - N, (q if A == 2 else None), (ql if A == 2 else None), nb


class Tempering:
    """The whole contract on the CPU: multispin_twin.bitsliced_sweep for the sweeps, measure, swap_pass and exchange above."""

    def __init__(self, planes, periodic, jr, jd, jl, T, seeds, swap_seeds, S):
        self.planes = np.array(planes, dtype=np.uint64)  # (R, A, W, D, Rr, C)
        self.periodic, self.j, self.T, self.S = periodic, (jr, jd, jl), [float(x) for x in T], S
        self.seeds = np.asarray(seeds, dtype=object).reshape(self.planes.shape[:2])
        self.swap_seeds = [int(x) for x in swap_seeds]
        self.book = Book(self.planes.shape[1], S, self.planes.shape[0])
        self.sweeps = 0

    def run(self, n_rounds, interval, swap=True):
        """Returns the recorded rows: unsat, sum (n, R, A, S), q, q_link (n, R, S) or None."""
        rows = []
        R, A = self.planes.shape[:2]
        for _ in range(n_rounds):
            for t in range(R):
                for a in range(A):
                    self.planes[t, a] = msc.bitsliced_sweep(self.planes[t, a], self.periodic, *self.j, self.T[t], interval,
                                                            int(self.seeds[t, a]), self.sweeps)
            self.sweeps += interval
            unsat, ssum, q, ql, nb = measure(self.planes, self.periodic, *self.j, self.S)
            rows.append((unsat, ssum, q, ql))
            if swap:
                accept = swap_pass(self.book, self.T, 2 * unsat - nb, self.swap_seeds)
                self.planes = exchange(self.planes, pack_masks(accept))
        cols = list(zip(*rows))
        return tuple(np.stack(c) if c and c[0] is not None else None for c in cols)


def exchange_unpacked(spins, accept):
    """spins (R, A, S, ...) of any dtype, accept (R - 1, A, S): every sample's configurations permuted on their own.  A new array."""
    out = np.array(spins)
    R, A, S = out.shape[:3]
    for a in range(A):
        for s in range(S):
            at = list(range(R))  # at[slot]: which of the input's slots the configuration came from
            for i in range(R - 1):
                if accept[i, a, s]:
                    at[i], at[i + 1] = at[i + 1], at[i]
            out[:, a, s] = np.asarray(spins)[at, a, s]
    return out

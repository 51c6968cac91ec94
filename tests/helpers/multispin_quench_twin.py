"""NumPy twin of K9's real-space correlations, two-time correlations and the xi_12 estimator (tsu_msc_c4 / _snapshot_overlap,
csrc/multispin_quench.hip; tsu.models.multispin_quench_3d).

Contract ("Real-space correlations and quench runs of multispin-coded glasses (K9)").  Per slot t and sample s
the site field is f = a b, the slot's two replicas, or f = s with one.  For a periodic axis d of length L and r = 0 .. L / 2,
C_d[r] = sum_x f_x f_{x + r e_d} over all N sites with wrap-around; an open axis has none.  The two-time correlation of a plane
against a snapshot is sum_x s_x(now) s_x(snap).

`c4_twin` and `two_time_twin` work on unpacked spins by np.roll products (the yardsticks).  `packed_c4` restates the count as the
kernel does it on packed words: the plan that cuts an axis into bundles of lines (whole rows for the column axis, slabs of up to 16
columns x the full axis for the other two), the staging of X = a ^ b (or a) into lines of L + 1 words, the lines a bundle holds, and
per (line, r) the set bits of X[x] ^ X[(x + r) mod L] per bit position; C = N - 2 count.  `xi12_twin` restates the estimator of
multispin_quench_3d with plain loops.
"""
import math

import numpy as np

ACC_WORDS, TARGET_WORDS, MAX_WORDS, SLAB, MAX_AXIS = 64 * 64, 4096, 16384, 16, 16382


def c4_twin(spin_array, periodic):
    """(C_z, C_r, C_c) from int8 spins (R, A, S, D, Rr, C): int64 (R, S, L_d / 2 + 1) per periodic axis, None for an open one."""
    s = np.asarray(spin_array).astype(np.int64)
    f = s[:, 0] * s[:, 1] if s.shape[1] == 2 else s[:, 0]
    out = []
    for d in range(3):
        if not periodic[d]:
            out.append(None)
            continue
        L = f.shape[2 + d]
        out.append(np.stack([(f * np.roll(f, -r, axis=2 + d)).sum(axis=(2, 3, 4)) for r in range(L // 2 + 1)], axis=-1))
    return tuple(out)


def two_time_twin(now, snap):
    """int64 (R, A, S): sum_x s_x(now) s_x(snap) from two int8 spin arrays (R, A, S, D, Rr, C)."""
    return (np.asarray(now).astype(np.int64) * np.asarray(snap).astype(np.int64)).sum(axis=(3, 4, 5))


def c4_plan(shape, periodic):
    """Per periodic axis d the kernel's launch plan: dict(L, D, sw, ncb, nunits, per, nb, G, npw, lds)."""
    depth, rows, cols = shape
    plan = {}
    for d in range(3):
        if not periodic[d]:
            continue
        L = shape[d]
        assert L <= MAX_AXIS
        a = {"L": L, "D": L // 2 + 1}
        a["G"] = min(a["D"], 64)
        a["npw"] = 64 // a["G"]
        if d == 2:
            a["sw"], a["ncb"], a["nunits"] = 1, 1, depth * rows
        else:
            sw = SLAB
            while sw > 1 and (sw * (L + 1) > MAX_WORDS or sw // 2 >= cols):
                sw //= 2
            a["sw"], a["ncb"] = sw, (cols + sw - 1) // sw
            a["nunits"] = (depth if d == 1 else rows) * a["ncb"]
        unit_words = a["sw"] * (L + 1)
        assert unit_words <= MAX_WORDS
        a["per"] = min(max(TARGET_WORDS // unit_words, 1), a["nunits"])
        a["nb"] = (a["nunits"] + a["per"] - 1) // a["per"]
        a["per"] = (a["nunits"] + a["nb"] - 1) // a["nb"]  # the bundles of equal size but the last
        a["lds"] = ACC_WORDS * 4 + a["per"] * unit_words * 8
        assert a["lds"] <= 160 * 1024
        plan[d] = a
    return plan


def _bundle_lines(x, d, a, b):
    """The lines (each (L,) uint64) that bundle b of axis d stages from the plane x (D, R, C) of X words, by the kernel's index maps;
    the words a bundle leaves unstaged belong to lines it skips."""
    depth, rows, cols = x.shape
    flat = x.ravel()
    L, sw, Lp = a["L"], a["sw"], a["L"] + 1
    u0 = b * a["per"]
    nu = min(a["per"], a["nunits"] - u0)
    nl = nu * sw
    lds = np.zeros(nl * Lp, np.uint64)
    staged = np.zeros(nl * Lp, bool)
    if d == 2:
        idx = np.arange(nu * L)
        li, xx = idx // L, idx % L
        lds[li * Lp + xx] = flat[u0 * L + idx]
        staged[li * Lp + xx] = True
        valid = np.ones(nl, bool)
    else:
        idx = np.arange(nl * L)
        j, q = idx & (sw - 1), idx // sw
        sl, xx = q // L, q % L
        unit = u0 + sl
        outer, c = unit // a["ncb"], (unit % a["ncb"]) * sw + j
        ok = c < cols
        i = np.where(d == 1, (outer * rows + xx) * cols + c, (xx * rows + outer) * cols + c)
        assert (i[ok] < flat.size).all() and (i[ok] >= 0).all()
        at = (sl * sw + j) * Lp + xx
        lds[at[ok]] = flat[i[ok]]
        staged[at[ok]] = True
        li = np.arange(nl)
        valid = (((u0 + li // sw) % a["ncb"]) * sw + li % sw) < cols
    lines = []
    for li in range(nl):
        if valid[li]:
            assert staged[li * Lp:li * Lp + L].all()
            lines.append(lds[li * Lp:li * Lp + L])
    return lines


def _bit_counts(words):
    """(64,) set bits per bit position of uint64 words."""
    b = np.unpackbits(np.ascontiguousarray(words, dtype="<u8").view(np.uint8).reshape(-1, 8), axis=1, bitorder="little")
    return b.sum(axis=0, dtype=np.int64)


def packed_c4(planes, periodic, S=None):
    """(C_z, C_r, C_c), int64 (R, 64 W or S, L_d / 2 + 1) or None, from the packed planes (R, A, W, D, Rr, C) alone."""
    planes = np.asarray(planes, dtype=np.uint64)
    R, A, W = planes.shape[:3]
    shape = planes.shape[3:]
    N = int(np.prod(shape))
    plan = c4_plan(shape, periodic)
    out = [np.zeros((R, 64 * W, shape[d] // 2 + 1), np.int64) if d in plan else None for d in range(3)]
    for t in range(R):
        for w in range(W):
            x = planes[t, 0, w] ^ planes[t, 1, w] if A == 2 else planes[t, 0, w]
            for d, a in plan.items():
                counts = np.zeros((a["D"], 64), np.int64)
                sites = 0
                for b in range(a["nb"]):
                    for line in _bundle_lines(x, d, a, b):
                        sites += line.size
                        for r in range(a["D"]):
                            counts[r] += _bit_counts(line ^ np.roll(line, -r))
                assert sites == N  # every site in exactly one line of one bundle
                out[d][t, 64 * w:64 * w + 64] = (N - 2 * counts).T
    return tuple(o if o is None or S is None else o[:, :S] for o in out)


def xi12_twin(c4, cut=3.0):
    """(xi12, xi12_error, r_cut) from per-sample correlators c4 (S, r_max + 1), with plain loops: mean and standard error over
    samples; r_cut = the last r before mean[r] < cut * error[r] for the first time, or r_max; xi12 = I_2 / I_1 with
    I_k = sum_{r <= r_cut} r^k mean[r]; the error by delete-one jackknife over samples with r_cut held fixed."""
    c4 = [[float(v) for v in row] for row in c4]
    S, R = len(c4), len(c4[0])

    def ratio(rows, r_cut):
        i1 = i2 = 0.0
        for r in range(r_cut + 1):
            m = sum(row[r] for row in rows) / len(rows)
            i1 += r * m
            i2 += r * r * m
        return i2 / i1 if i1 != 0.0 else float("nan")

    r_cut = R - 1
    if S >= 2:
        for r in range(R):
            m = sum(row[r] for row in c4) / S
            var = sum((row[r] - m) ** 2 for row in c4) / (S - 1)
            if m < cut * math.sqrt(var / S):
                r_cut = r - 1
                break
    xi = ratio(c4, r_cut)
    if S < 2:
        return xi, float("nan"), r_cut
    th = [ratio(c4[:i] + c4[i + 1:], r_cut) for i in range(S)]
    mean_th = sum(th) / S
    return xi, math.sqrt((S - 1) / S * sum((v - mean_th) ** 2 for v in th)), r_cut

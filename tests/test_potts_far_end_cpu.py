"""What tests/test_potts_far_end_gpu.py rests on, checked on the host (no GPU needed): the Potts positions of the far-end table
(tests/helpers/far_end.py), `lo_decided` of the two Potts twins against a plain-Python evaluation of the rule from `chain`'s
arithmetic, the pinned counts of the sites that the low half of u decides, and the two half-sweeps in which one octet holds two of
them (tools/potts_lo_pair_search.py finds those)."""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fe = _load("far_end")
pt = _load("potts_twin")
p3 = _load("potts3d_twin")
FIELDS = {2: (0.0, 0.25), 3: (0.3, 0.0, -0.2), 5: (0.1, -0.3, 0.2, 0.0, 0.4), 8: fe.POTTS_FIELD8}


def test_the_potts_positions_are_what_the_issue_states():
    pos = dict(fe.potts_positions(5))
    assert pos == {"hs_sign": 2 ** 30 - 3, "hs_wrap": 2 ** 31 - 3, "sweep_wrap": 2 ** 32 - 3}
    s = pos["hs_sign"]
    assert 2 * s < 2 ** 31 <= 2 * (s + 4) + 1                      # hs crosses the sign bit inside 5 sweeps
    s = pos["hs_wrap"]
    assert s + 4 < 2 ** 32 and 2 * s < 2 ** 32 <= 2 * (s + 4) + 1  # hs wraps, the sweep counter does not
    s = pos["sweep_wrap"]
    assert s < 2 ** 32 <= s + 4                                    # the sweep counter wraps
    lo = fe.POTTS_LO_MODEL
    assert 2 * lo["sweep0"] < 2 ** 31 <= 2 * (lo["sweep0"] + lo["n_sweeps"] - 1) + 1 and lo["replica"] == fe.REPLICA_MAX
    assert fe.POTTS_FIELD8 == (0.5, -0.5, 0.25, 0.0, -0.25, 0.1, -0.1, 0.3)
    # T = 0.01 J of the spanning-cluster tests: -expm1(-100) rounds to 1, so the bond threshold is 2^32 itself (the kernels compare
    # in 64 bits) and every bond between equal colours is active
    assert pt.threshold(1.0, 0.01) == 2 ** 32 == p3.threshold(2.5, 0.025)


def _plain_lo_decided(twin, spins, q, periodic, J, h, T, hs, seed, replica):
    """The rule of `chain`, site by site in Python floats and integers: the sites of colour hs & 1 whose colour at
    u & 0xFFFF0000 differs from the one at u | 0xFFFF."""
    s0 = np.asarray(spins)
    shape = s0.shape
    E, F = (a.tolist() for a in twin.tables(q, J, h, T))
    if s0.ndim == 2:
        nbs = twin._site_lists(shape[0], shape[1], periodic)
        col_of = ((np.arange(shape[0])[:, None] + np.arange(shape[1])[None, :]) & 1).ravel().tolist()
        U = twin._uniform_block(shape[0], shape[1], hs >> 1, 1, seed, replica)[hs & 1]
    else:
        nbs = twin._site_lists(shape, periodic)
        col_of = twin.colours(shape).ravel().tolist()
        U = twin._uniform_block(shape, hs >> 1, 1, seed, replica)[hs & 1]
    s = s0.ravel().tolist()
    out = np.zeros(s0.size, bool)
    for i in range(s0.size):
        if col_of[i] != (hs & 1):
            continue
        cnt = [0] * q
        for j in nbs[i]:
            cnt[s[j]] += 1
        Z, acc = [], 0.0
        for c in range(q):
            w = E[cnt[c]] * F[c]
            acc = w if c == 0 else acc + w
            Z.append(acc)
        picked = []
        for u in (U[i] & 0xFFFF0000, U[i] | 0xFFFF):
            lhs = float(u) * Z[q - 1]
            new = q - 1
            for c in range(q - 1):
                if lhs < Z[c] * 4294967296.0:
                    new = c
                    break
            picked.append(new)
        out[i] = picked[0] != picked[1]
    return out.reshape(shape)


# (twin, shape, periodic, q, J, h, T, first half-sweep): 400 half-sweeps each from one random state.  The sites found are listed
# so that the comparison cannot pass on empty masks (about (q - 1) 2^-16 of the sites are decided by the low half)
LO_TINY = [(pt, (6, 34), True, 8, 1.0, FIELDS[8], 1.0, 2 ** 31 - 200), (pt, (5, 7), False, 3, -1.0, FIELDS[3], 0.7, 2 ** 32 - 400),
           (p3, (4, 3, 18), (True, False, True), 5, 0.37, FIELDS[5], 2.0, 2 ** 31 - 200), (p3, (2, 2, 34), p3.ALL, 8, 1.0, None, 0.9, 7)]


@pytest.mark.parametrize("case", LO_TINY, ids=lambda c: "x".join(map(str, c[1])) + f"-q{c[3]}")
def test_lo_decided_against_plain_python(case):
    twin, shape, per, q, J, h, T, hs0 = case
    s = np.random.default_rng(11).integers(0, q, size=shape).astype(np.int8)
    found = 0
    for hs in range(hs0, hs0 + 400):
        got = twin.lo_decided(s, q, per, J, h, T, hs, fe.SEED_HI, fe.REPLICA_MAX)
        want = _plain_lo_decided(twin, s, q, per, J, h, T, hs, fe.SEED_HI, fe.REPLICA_MAX)
        assert got.dtype == np.bool_ and got.shape == shape and (got == want).all(), hs
        found += int(got.sum())
    print(f"\n{shape} q={q}: {found} sites decided by the low half in 400 half-sweeps")
    assert found >= 1


@pytest.mark.parametrize("twin,shape,per", [(pt, (6, 34), True), (p3, (4, 3, 18), (True, False, True))], ids=["2d", "3d"])
def test_lo_trajectory_is_the_sweep_with_the_masks_of_its_states(twin, shape, per):
    q, J, h, T = 5, 1.0, FIELDS[5], 0.8
    s = np.random.default_rng(12).integers(0, q, size=shape).astype(np.int8)
    sweep0 = fe.POTTS_SWEEP_WRAP
    end, masks = twin.lo_trajectory(s, q, per, J, h, T, 5, fe.SEED_HI, sweep0, fe.REPLICA_BYTES)
    assert (end == twin.sweep(s, q, per, J, h, T, 5, fe.SEED_HI, sweep0, fe.REPLICA_BYTES)).all() and len(masks) == 10
    for k in range(5):  # the masks at the start of every sweep, from the state `sweep` gives there
        state = twin.sweep(s, q, per, J, h, T, k, fe.SEED_HI, sweep0, fe.REPLICA_BYTES)
        hs = (2 * ((sweep0 + k) % 2 ** 32)) % 2 ** 32
        assert (masks[2 * k] == twin.lo_decided(state, q, per, J, h, T, hs, fe.SEED_HI, fe.REPLICA_BYTES)).all()


def test_lo_fold_counts_positions_and_octets():
    mask = np.zeros((2, 3, 40), bool)
    mask[0, 1, 0] = mask[0, 1, 5] = True      # global row 1, octet 0: positions 0 and 2
    mask[1, 2, 33] = True                     # global row 5, octet 2: position 0
    mask[1, 0, 31] = mask[1, 0, 32] = True    # global row 3: the last site of octet 1 (position 7), the first of octet 2
    per_m, pairs = pt.lo_fold(mask)
    assert per_m == [3, 0, 1, 0, 0, 0, 0, 1] and pairs == 1
    oct_ = p3.lo_octets(mask)
    assert oct_.shape == (6, 3) and oct_[1, 0] == 2 and oct_[5, 2] == 1 and oct_[3, 1] == 1 and oct_[3, 2] == 1 and oct_.sum() == 5


def lo_case_counts(twin, shape):
    """The low-half case of the far-end table on `shape` (periodic): (start, final state, sites decided by the low half per octet
    position over the 4 half-sweeps, octets with two of them)."""
    m = fe.POTTS_LO_MODEL
    start = np.random.default_rng(7).integers(0, m["q"], size=shape).astype(np.int8)
    end, masks = twin.lo_trajectory(start, m["q"], True, m["J"], m["h"], m["T"], m["n_sweeps"], m["seed"], m["sweep0"], m["replica"])
    per_m, pairs = np.zeros(8, np.int64), 0
    for mask in masks:
        a, b = twin.lo_fold(mask)
        per_m += np.array(a)
        pairs += b
    return start, end, per_m.tolist(), pairs


# the twin's counts, which the GPU test recomputes and requires to be at least 4 at every position before it compares the device
LO_COUNTS = {"3d": [14, 19, 20, 9, 15, 17, 16, 15], "2d": [16, 12, 17, 19, 7, 17, 22, 6]}


@pytest.mark.parametrize("dim", ["3d", "2d"])
def test_the_low_half_case_reaches_every_octet_position(dim):
    """34 x 128 x 128 and 1024 x 544, q = 8, J = 1, h = FIELDS[8], T = 1, SEED_HI, sweep0 = 2^30 - 1, replica 2^24 - 1, 2 sweeps from
    default_rng(7): the low half decides 125 sites in 3-D (9 .. 20 per octet position m) and 116 in 2-D (6 .. 22), never two in
    one octet."""
    twin, shape = (p3, fe.POTTS_LO_SHAPE_3D) if dim == "3d" else (pt, fe.POTTS_LO_SHAPE_2D)
    _, _, per_m, pairs = lo_case_counts(twin, shape)
    print(f"\n{shape}: per position {per_m}, {sum(per_m)} in all, {pairs} octets with two")
    assert min(per_m) >= 4
    assert per_m == LO_COUNTS[dim] and pairs == 0


@pytest.mark.parametrize("sweep,colour,rho,octet", fe.POTTS_LO_PAIRS)
def test_two_low_half_sites_in_one_octet(sweep, colour, rho, octet):
    """J = 0: the sums do not depend on the state, so the octets are the same from any start, in 2-D and on the 3-D lattice with
    the same 128 global rows (where the colouring of the odd layers picks the other column parity of the same positions)."""
    m = fe.POTTS_LO_PAIR_MODEL
    hs = 2 * sweep + colour
    for twin, shape in ((pt, fe.POTTS_LO_PAIR_SHAPE_2D), (p3, fe.POTTS_LO_PAIR_SHAPE_3D)):
        for rng_seed in (7, 8):
            s = np.random.default_rng(rng_seed).integers(0, m["q"], size=shape).astype(np.int8)
            mask = twin.lo_decided(s, m["q"], True, m["J"], m["h"], m["T"], hs, m["seed"], m["replica"])
            per_octet = twin.lo_octets(mask)
            assert per_octet.shape == (128, 8) and per_octet[rho, octet] >= 2, (shape, per_octet[rho].tolist())
            assert (twin.lo_decided(s, m["q"], True, m["J"], m["h"], m["T"], hs ^ 1, m["seed"], m["replica"]) & mask).sum() == 0

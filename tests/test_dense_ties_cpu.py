"""The near-tie generators of the oracle (oracle.dense_tie_chain, oracle.dense_tie_bias) on the CPU: every generated chain is the
reference's own loop (the C replay and the NumPy restatement, both pinned by golden vectors), every placement class lands where
it claims, the clamp ladder gives the hand-derived outcomes, and a Philox-crafted first sweep is the oracle's Philox sweep.
tests/test_dense_ties_gpu.py drives the dense kernels with these chains."""
import numpy as np
import pytest

from oracle import oracle as ora


def _chain(n, seed, temps, sym=True, bias=True, ladder=0, order=False):
    J, b, _ = ora.dyadic_system(n, seed, sym=sym, bias=bias, ladder=ladder, rounding=16 if ladder else 0)
    rng = np.random.default_rng(seed + 1)
    o = np.array([rng.permutation(n) for _ in temps]) if order else None
    ch = ora.dense_tie_chain(J, b, temps, order=o, rng=rng, ladder=ladder)
    return J, b, o, ch


@pytest.mark.parametrize("n,sym,bias,ladder,order,temps", [
    (1, True, True, 0, False, [0.5, 1.0, 0.7]),
    (65, True, True, 16, False, [0.5, 0.7, 1.0, 0.5]),
    (96, False, False, 16, True, [0.5, 2.0, 0.7]),
    (300, False, True, 16, True, [0.7, 0.5, 0.25]),
    (129, True, True, 16, False, list(np.linspace(4.0, 0.25, 70))),
])
def test_chain_is_the_reference_loop(n, sym, bias, ladder, order, temps):
    J, b, o, ch = _chain(n, 7 * n, temps, sym, bias, ladder, order)
    u, states = ch["uniforms"], ch["states"]
    for t, T in enumerate(temps):
        ot = None if o is None else o[t:t + 1]
        c = ora.c_dense_sweep_replay(states[t], J, b, T, u[t:t + 1], ot)
        np.testing.assert_array_equal(c, states[t + 1])
        r = ora.ref_gibbs_sweep(states[t].astype(np.int64), J, b, T, u[t:t + 1], ot)
        np.testing.assert_array_equal(r, states[t + 1])
    if len(set(temps)) == 1:
        np.testing.assert_array_equal(ora.c_dense_sweep_replay(states[0], J, b, temps[0], u, o), states[-1])
    assert np.all(u >= 0.0) and np.all(u < 1.0) and np.all(u * 2.0 ** 53 == np.floor(u * 2.0 ** 53))


def test_exact_grid_fields_and_energies():
    J, b, K = ora.dyadic_system(200, 3, sym=False)
    assert np.all(np.diag(J) != 0) and ora.energy_is_exact(J, b)
    assert np.all(J.astype(np.float32).astype(np.float64) == J)
    s = np.random.default_rng(0).integers(0, 2, 200)
    # any summation order gives the same field: forwards, backwards, pairwise
    f = J @ s + b
    f2 = np.array([sum(J[i, j] * s[j] for j in reversed(range(200))) + b[i] for i in range(200)])
    np.testing.assert_array_equal(f, f2)
    assert ora.c_dense_energy(s, J, b) == ora.ref_compute_energy(s[::-1][::-1], J, b)
    Jl, bl, _ = ora.dyadic_system(64, 3, ladder=16)
    assert not ora.energy_is_exact(Jl, bl)  # ladder biases are off the grid
    assert np.all(Jl[:16] == 0) and np.any(Jl[16:, :16] != 0)


def test_every_class_lands_in_its_band_with_both_outcomes_and_all_transitions():
    temps = [0.5, 0.7, 1.0, 0.5, 2.0, 0.25]
    J, b, o, ch = _chain(400, 11, temps, sym=False, ladder=16, order=True)
    cls, x, u, states = ch["cls"], ch["x"], ch["uniforms"], ch["states"]
    before = np.stack([states[t][o[t]] for t in range(len(temps))])
    after = np.stack([states[t + 1][o[t]] for t in range(len(temps))])
    for c in "ABCDEF":
        assert np.any(cls == c, axis=1)[[t for t, T in enumerate(temps) if c not in "DF" or T == 0.5]].all(), c
    for c in "ABCE":
        m = cls == c
        for out in (0, 1):
            assert np.sum(m & (after == out)) >= 20, (c, out)
        assert np.sum(m & (before == 0) & (after == 1)) >= 10
        assert np.sum(m & (before == 1) & (after == 0)) >= 10
        assert np.sum(m & (before == after)) >= 10
    for t, k in zip(*np.nonzero(cls != "R")):
        c, xx, uu = cls[t, k], x[t, k], u[t, k]
        got, dist = ora.classify(xx, uu)
        lg = ora.logit(uu)
        if c == "A":  # inside the float64 band with room to spare, and 64 ... 1024 units of 2^-53 from p
            assert got == "A" and dist <= 0.5 * ora.BAND_EXACT * (1 + abs(lg))
            assert 63 * ora.U53 <= abs(uu - ora._sig(xx)) <= 1025 * ora.U53
        elif c == "B":  # outside the float64 band by a factor two at least, well inside the float band
            assert got == "B" and 2 * ora.BAND_EXACT * (1 + abs(lg)) <= dist <= 0.1 * ora.BAND_FLOAT * (1 + abs(lg))
        elif c == "C":  # just outside the float band (the kernels' float logit errs by < 1e-5 (1 + |logit|))
            assert got == "C" and 1.5 * ora.BAND_FLOAT * (1 + abs(lg)) <= dist <= 3 * ora.BAND_FLOAT * (1 + abs(lg))
        elif c == "D":
            assert temps[t] == 0.5 and xx in ora.LADDER_X
        elif c == "E":
            assert uu in ora.EXTREME_U
        elif c == "F":  # the reference's rounded sigmoid decides against the exact comparison, inside the float64 band
            assert got == "A" and (1 if uu < ora.c_sigmoid(xx) else 0) != (1 if xx > lg else 0)
    f = (cls == "F") & (x >= 10)
    assert np.sum(f & (after == 0)) >= 10 and np.sum(f & (after == 1)) >= 10
    # class E at moderate and at clamped x
    ex = np.abs(x[cls == "E"])
    assert np.any(ex < 5) and np.any(ex > 20)


def test_clamp_ladder_gives_the_hand_derived_outcomes():
    assert ora.ladder_u(20.0) == 1 - 2.0 ** -30 and ora.ladder_u(-20.0) == 2.0 ** -30
    hand = {20.0: 0, 20.0 + 2.0 ** -40: 1, -20.0: 1, -20.0 - 2.0 ** -40: 0, 25.0: 1, -25.0: 0,
            20.0 - 2.0 ** -40: 0, -20.0 + 2.0 ** -40: 1, 20.0 + 5e-4: 1, 20.0 - 5e-4: 0, -20.0 - 5e-4: 0, -20.0 + 5e-4: 1,
            20.0 + 2e-3: 1, 20.0 - 2e-3: 0, -20.0 - 2e-3: 0, -20.0 + 2e-3: 1}
    assert set(hand) == set(ora.LADDER_X)
    for x, want in hand.items():
        u = ora.ladder_u(x)
        assert (1 if u < ora.c_sigmoid(x) else 0) == want, x
        assert (1 if u < ora.ref_sigmoid(x) else 0) == want, x
        if abs(x) > 20:  # clamped and unclamped sigmoid disagree here: the clamp decides
            assert (1 if u < 1.0 / (1.0 + np.exp(-x)) else 0) != want, x
        elif abs(x) == 20:  # on the clamp: not clamped (strict >), a >= clamp would give the other outcome
            assert (1 if u < (1.0 if x > 0 else 0.0) else 0) != want, x
    # in a chain: every ladder visit at T = 0.5 gives those outcomes, whatever the state before
    J, b, o, ch = _chain(64, 5, [0.5, 0.5, 1.0, 0.5], ladder=16)
    for t in (0, 1, 3):
        for i in range(16):
            assert ch["cls"][t, i] == "D" and ch["x"][t, i] == ora.LADDER_X[i]
            assert ch["states"][t + 1][i] == hand[ora.LADDER_X[i]]
    np.testing.assert_array_equal(ora.c_dense_sweep_replay(ch["states"][0], J, b, 0.5, ch["uniforms"][:2]), ch["states"][2])


@pytest.mark.parametrize("n,T,order,sym", [(1, 0.7, False, True), (64, 0.5, False, False), (300, 0.7, True, True),
                                           (2048, 1.0, False, False), (452, 0.7, True, False)])
def test_philox_crafted_first_sweep_is_the_oracle_philox_sweep(n, T, order, sym):
    J, _, _ = ora.dyadic_system(n, n + 3, sym=sym, bias=False)
    rng = np.random.default_rng(n)
    s0 = rng.integers(0, 2, n).astype(np.int8)
    o = rng.permutation(n) if order else None
    seed, sweep0, replica = (1 << 33) + 12345, 7, 3
    b, cls, s1 = ora.dense_tie_bias(J, T, o, seed, sweep0, replica, s0, rng=rng)
    assert not np.all(b * 2.0 ** 20 == np.floor(b * 2.0 ** 20))  # off the couplings' grid
    np.testing.assert_array_equal(ora.dense_sweep_philox(s0, J, b, T, 1, seed, sweep0=sweep0, replica=replica,
                                                         order=None if o is None else o[None]), s1)
    if n >= 300:
        for c in "ABC":
            assert np.sum(cls == c) >= n // 5, c
    # every crafted site lands in its band against its own Philox uniform (both key words, the sweep and the replica tag matter)
    s = s0.astype(np.float64).copy()
    visit = range(n) if o is None else o
    for k, i in enumerate(visit):
        u = ora.dense_uniform(i, sweep0, seed, replica)
        x = (float(J[i] @ s) + b[i]) / T
        got, _ = ora.classify(x, u)
        if cls[k] != "R":
            assert got == cls[k], (k, cls[k], got)
            other = [ora.dense_uniform(i, sweep0 + 1, seed, replica), ora.dense_uniform(i, sweep0, seed, replica ^ 1),
                     ora.dense_uniform(i, sweep0, seed & 0xFFFFFFFF, replica)]
            assert all(v != u for v in other)
        s[i] = s1[i]

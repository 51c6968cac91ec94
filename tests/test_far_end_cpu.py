"""The NumPy twins that tests/test_far_end_gpu.py compares the kernels with, checked against the C oracle at the far-end table's own
seeds, counters and replica ids (tests/helpers/far_end.py), and the range checks of the ctypes wrappers.  No GPU.

The oracle takes uint64 seeds and uint32 counters and is pinned by the Philox known-answer vectors with all-ones counters
(tests/test_oracle_golden.py); a twin that kept a counter above 32 bits, or dropped seed >> 32, would differ from it here."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import oracle as ora

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fe = _load("far_end")
k7 = _load("disorder_twin")
k8 = _load("lattice3d_twin")
sw2 = _load("cluster_twin")
sw3 = _load("cluster3d_twin")
swf = _load("cluster_field_twin")
lv = _load("langevin_twin")

SEEDS = (fe.SEED_HI, fe.SEED_CARRY, fe.SEED_CARRY + 2, fe.SEED_CARRY + 3)   # (+ 2: the carry has happened; + 3: k0 = 1, k1 = 1)
HALF_SWEEPS = (2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 2, 2 ** 32 - 1)
COUNTERS = (2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1)


def _key(seed):
    return np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32)


def _oracle_word(c0, c1, c2, c3, seed):
    return [int(w) for w in ora.philox4x32_10(np.array([c0, c1, c2, c3], np.uint32), _key(seed))]


def test_the_table_is_what_the_issue_states():
    assert fe.SEED_HI == 0xFEDCBA9876543210 and fe.SEED_HI >> 63 == 1 and fe.SEED_HI & 0xFFFFFFFF not in (0, fe.SEED_HI >> 32)
    assert fe.SEED_CARRY < 2 ** 32 <= fe.SEED_CARRY + 2
    assert fe.REPLICAS == (2 ** 24 - 1, 0xABCDEF)
    for n in (4, 5, 19):
        assert 2 * (fe.end(n) + n - 1) + 1 == 2 ** 32 - 1                         # the last half-sweep of a call that ends at the limit
        assert 2 * fe.straddle(n) < 2 ** 31 <= 2 * (fe.straddle(n) + n - 1) + 1    # hs crosses the sign bit inside the call
        assert fe.end32(n) + n - 1 == 2 ** 32 - 1
        assert fe.straddle32(n) < 2 ** 31 <= fe.straddle32(n) + n - 1


def test_vectorised_philox_at_far_end_keys_and_counters():
    """cluster_twin.philox4x32_10 (under every lattice and cluster twin) and langevin_twin.philox4x32_10."""
    ctrs = [(c0, c1, c2, tag | (rep << 8)) for c0 in (0, 3, 2 ** 26) for c1 in (0, 2 ** 31 - 1) for c2 in COUNTERS + HALF_SWEEPS
            for tag in (0, 1, 6, 12) for rep in fe.REPLICAS]
    a = np.array(ctrs, dtype=np.uint64)
    for seed in SEEDS:
        got = sw2.philox4x32_10(a[:, 0], a[:, 1], a[:, 2], a[:, 3], seed & 0xFFFFFFFF, seed >> 32)
        got_lv = lv.philox4x32_10(a.astype(np.uint32), _key(seed))
        for i, c in enumerate(ctrs):
            want = _oracle_word(*c, seed)
            assert [int(g[i]) for g in got] == want, (c, hex(seed))
            assert [int(v) for v in got_lv[i]] == want, (c, hex(seed))


@pytest.mark.parametrize("rows,cols", [(5, 7), (3, 40), (1, 9)])
def test_site_uniforms_of_the_lattice_twins(rows, cols):
    """K7's twin (and K8's, which reshapes it) against the oracle's site uniforms: every half-sweep of the table, SEED_HI and the
    carried seeds, both replica ids."""
    for hs in HALF_SWEEPS:
        for seed in SEEDS:
            for rep in fe.REPLICAS:
                want = ora.ising2d_site_uniforms(rows, cols, hs, seed, rep)
                assert (k7.site_uniforms(rows, cols, hs, seed, rep) == want).all(), (hs, hex(seed), rep)
    want = ora.ising2d_site_uniforms(3 * rows, cols, 2 ** 32 - 1, fe.SEED_HI, fe.REPLICA_MAX)
    assert (k8.site_uniforms((3, rows, cols), 2 ** 32 - 1, fe.SEED_HI, fe.REPLICA_MAX) == want.reshape(3, rows, cols)).all()


@pytest.mark.parametrize("rows,cols,periodic", [(6, 10, True), (5, 7, False)])
def test_k7_and_k8_twins_sweep_like_the_oracle_at_the_far_end(rows, cols, periodic):
    """With constant couplings and field the K7 rule is K1's (threshold table of set_model): the twins' sweeps across hs = 2^31 and up
    to hs = 2^32 - 1 equal ora.ising2d_sweep with the same counters.  A twin that formed hs beyond 32 bits would draw other words."""
    J, h, T = 1.0, 0.25, 2.0
    table = ora.ising2d_thresholds(J, h, T, 0)
    jr, jd, hh = k7.uniform_disorder(rows, cols, periodic, J, h)
    s = ora.ising2d_randomize(rows, cols, fe.SEED_HI, fe.REPLICA_BYTES)
    for name, sweep0 in fe.lattice_positions(5):
        want = ora.ising2d_sweep(s, periodic, table, 5, fe.SEED_HI, sweep0, fe.REPLICA_MAX)
        got = k7.sweep(s, periodic, jr, jd, hh, T, 5, fe.SEED_HI, sweep0, fe.REPLICA_MAX)
        assert (got == want).all(), name
        z = np.zeros((1, rows, cols), np.float32)
        got3 = k8.sweep(s[None], (False, periodic, periodic), jr[None], jd[None], z, hh[None], T, 5, fe.SEED_HI, sweep0, fe.REPLICA_MAX)
        assert (got3[0] == want).all(), name
        s = want


def test_cluster_twins_draw_the_oracles_words():
    """Bond, layer, flip and ghost words of the cluster twins at step counters 2^31 - 1, 2^31 and 2^32 - 1."""
    shape = (2, 3, 10)
    D, R, C = shape
    for t in COUNTERS:
        for seed in (fe.SEED_HI, fe.SEED_CARRY + 3):
            for rep in fe.REPLICAS:
                ur, ud, ul = sw3.bond_uniforms(shape, seed, t, rep)
                ug = swf.ghost_uniforms(shape, seed, t, rep)
                flips = sw3.flip_of_roots(np.arange(D * R * C), C, seed, t, rep)
                for rho in range(D * R):
                    for c in range(C):
                        z, r = divmod(rho, R)
                        wb = _oracle_word(c >> 1, rho, t, sw3.TAG_SW_BOND | (rep << 8), seed)
                        assert (int(ur[z, r, c]), int(ud[z, r, c])) == (wb[2 * (c & 1)], wb[2 * (c & 1) + 1])
                        assert int(ul[z, r, c]) == _oracle_word(c >> 2, rho, t, sw3.TAG_SW_LAYER | (rep << 8), seed)[c & 3]
                        assert int(ug[z, r, c]) == _oracle_word(c >> 2, rho, t, swf.TAG_SW_GHOST | (rep << 8), seed)[c & 3]
                        assert bool(flips[rho * C + c]) == bool(_oracle_word(c >> 2, rho, t, sw3.TAG_SW_FLIP | (rep << 8), seed)[c & 3] >> 31)
    # the 2-D twin's step is the one-layer 3-D twin's with constant J (same words, same roots)
    s = ora.ising2d_randomize(6, 10, fe.SEED_HI, fe.REPLICA_MAX)
    one = np.ones((1, 6, 10), np.float32)
    for step0 in (fe.straddle32(4), fe.end32(4)):
        a = sw2.sweep(s, True, 1.0, 2.269, 4, fe.SEED_HI, step0, fe.REPLICA_BYTES)
        b = sw3.sweep(s[None], (False, True, True), one, one, 0 * one, 2.269, 4, fe.SEED_HI, step0, fe.REPLICA_BYTES)
        assert (a == b[0]).all()


def test_dense_uniform_uses_both_key_words_and_the_whole_counter():
    """ora.dense_uniform (K2's and K5's 53-bit uniform) from the oracle's own Philox: word pair (i & 1) of
    Philox(i >> 1, 0, t, TAG_DENSE | replica << 8)."""
    for t in COUNTERS:
        for seed in SEEDS:
            for rep in fe.REPLICAS:
                for i in (0, 1, 4099, 40007):
                    w = _oracle_word(i >> 1, 0, t, 4 | (rep << 8), seed)
                    u = ora.dense_uniform(i, t, seed, rep)
                    a, b = w[2 * (i & 1)] >> 5, w[2 * (i & 1) + 1] >> 6
                    assert u * 2.0 ** 53 == a * 2 ** 26 + b, (i, t, hex(seed), rep)
                    assert u != ora.dense_uniform(i, t, seed & 0xFFFFFFFF, rep) or seed >> 32 == 0
                    assert u != ora.dense_uniform(i, t, seed, rep & 0xFFFF)
                    assert u != ora.dense_uniform(i, t & 0x7FFFFFFF, seed, rep) or t < 2 ** 31


def test_wrapper_range_checks():
    """The ctypes wrappers refuse what does not fit the C type instead of letting ctypes wrap it (tsu/_hip.py)."""
    from tsu import _hip
    assert _hip.REPLICA_LIMIT == fe.REPLICA_LIMIT
    assert _hip._seed(fe.SEED_HI) == fe.SEED_HI and _hip._seed(2 ** 64 - 1) == 2 ** 64 - 1 and _hip._seed(np.uint64(7)) == 7
    assert _hip._counter("sweep0", 2 ** 32 - 1) == 2 ** 32 - 1 and _hip._replica(fe.REPLICA_MAX) == fe.REPLICA_MAX
    for bad in (lambda: _hip._seed(2 ** 64), lambda: _hip._seed(-1), lambda: _hip._counter("sweep0", 2 ** 32),
                lambda: _hip._counter("step0", -1), lambda: _hip._replica(2 ** 24), lambda: _hip._replica(2 ** 32 + 3),
                lambda: _hip._replica(-1)):
        with pytest.raises(ValueError):
            bad()
    a = _hip._uint_array("seeds", [1, fe.SEED_HI, np.uint64(2 ** 64 - 1)], np.uint64)
    assert a.dtype == np.uint64 and [int(v) for v in a] == [1, fe.SEED_HI, 2 ** 64 - 1]
    assert _hip._uint_array("replicas", np.array([0, fe.REPLICA_MAX]), np.uint32, _hip.REPLICA_LIMIT).tolist() == [0, fe.REPLICA_MAX]
    for bad in (lambda: _hip._uint_array("sweep0s", [0, 2 ** 32], np.uint32), lambda: _hip._uint_array("seeds", [2 ** 64], np.uint64),
                lambda: _hip._uint_array("seeds", [-1], np.uint64),
                lambda: _hip._uint_array("replicas", [0, 2 ** 24], np.uint32, _hip.REPLICA_LIMIT)):
        with pytest.raises(ValueError):
            bad()


def test_the_header_states_the_limits_and_declares_the_query():
    from tsu import _hip
    root = os.path.dirname(HERE)
    with open(os.path.join(root, "include", "tsu_hip.h")) as f:
        text = f.read()
    assert "int tsu_ising2d_strip_numbering(tsu_ising2d* lat, uint32_t* generation, uint64_t* restarts);" in text
    assert "tsu_ising2d_strip_numbering" in _hip.SIGNATURES
    assert "below 2^24" in text and "sweep0 + n_sweeps <= 2^31" in text and "<= 2^32" in text

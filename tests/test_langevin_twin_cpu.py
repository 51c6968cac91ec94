"""The float64 twin of K3's noise stream (tests/helpers/langevin_twin.py) against the oracle: the same Philox words, the oracle's
float32 Box-Muller within float32 libm error of the twin's float64 one, and the uint32 wrap of the chain and step counters."""
import importlib.util
import os

import numpy as np

from oracle import oracle as ora

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("langevin_twin", os.path.join(HERE, "helpers", "langevin_twin.py"))
twin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(twin)

KATS = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
        ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
        ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
         (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


def test_twin_philox_known_answers_and_random_counters():
    for ctr, key, want in KATS:
        got = twin.philox4x32_10(np.array([ctr], dtype=np.uint32), key)[0]
        assert tuple(int(v) for v in got) == want
        np.testing.assert_array_equal(got, ora.philox4x32_10(ctr, key))
        # the same through words(): key = seed low / high
        got = twin.words(ctr[0], ctr[1], ctr[2], ctr[3], key[0] | (key[1] << 32))
        assert tuple(int(v) for v in got) == want
    rng = np.random.default_rng(0)
    ctrs = rng.integers(0, 2 ** 32, size=(1000, 4), dtype=np.uint64).astype(np.uint32)
    key = np.array([123456789, 987654321], dtype=np.uint32)
    want = np.array([ora.philox4x32_10(c, key) for c in ctrs])
    np.testing.assert_array_equal(twin.philox4x32_10(ctrs, key), want)


def test_oracle_normals_are_the_twins_within_float32_libm_error():
    """The oracle's float32 restatement against float64 at 10^4 random counters of both tags.  Bound: |xi| <= r <= 5.77 (u1 >= 2^-24);
    the float32 angle 2 pi u2 carries up to half an ulp of 2 pi (2.4e-7) twice over (the product's rounding and the constant's), the
    radius half an ulp each from log, the product and the root, cos / sin under an ulp: |error| <= r (4.8e-7 + 3 * 6e-8) + 6e-8 r
    <= 7.2e-7 r + ulp(xi), under 4.5e-6 at the largest radius."""
    rng = np.random.default_rng(1)
    n = 10000
    q, chain, step = (rng.integers(0, 2 ** 32, size=n, dtype=np.uint64) for _ in range(3))
    seed = 0x9E3779B97F4A7C15
    for tag in (twin.TAG_LANGEVIN, twin.TAG_LANGEVIN_RESTART):
        xi, r, ang = twin.normals_f64(q, chain, step, tag, seed)
        got = np.array([ora.langevin_normals_f32(int(q[i]), int(chain[i]), int(step[i]), seed, tag) for i in range(n)], dtype=np.float64)
        err = np.abs(got - xi)
        bound = 7.2e-7 * np.repeat(r, 2, axis=-1) + 2.4e-7 * np.maximum(np.abs(xi), 1.0)
        assert np.all(err <= bound), (float(err.max()), int(np.argmax(err / bound)))
        assert float(err.max()) <= 4.5e-6
        # r and the angle are the pair's polar coordinates
        np.testing.assert_allclose(np.hypot(xi[:, 0::2], xi[:, 1::2]), r, rtol=1e-14)
        assert np.all((ang >= 0.0) & (ang < 2.0 * np.pi)) and np.all(r >= 0.0) and float(r.max()) <= np.sqrt(48 * np.log(2.0))


def test_twin_step_is_the_oracles_within_float32():
    rng = np.random.default_rng(2)
    x = rng.normal(size=(3, 9)).astype(np.float32)
    k = rng.uniform(0.5, 2.0, size=9).astype(np.float32)
    mu = rng.normal(size=9).astype(np.float32)
    want, wtraj = ora.langevin_quadratic_f32(x, k, mu, 6, 0.02, 1.5, 0.7, 99, step0=3, chain0=5, trajectory=True)
    got, traj = twin.quadratic_f64(x, k, mu, 6, 0.02, 1.5, 0.7, 99, step0=3, chain0=5, trajectory=True)
    # six steps, each: two float32 roundings of a state of size <= 8 (2 * 4.8e-7) and a normal's error scaled by 0.137
    np.testing.assert_allclose(traj, wtraj, rtol=0, atol=6 * (1e-6 + 0.137 * 4.5e-6))
    np.testing.assert_array_equal(traj[-1], got)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)
    # the restart stream
    r = twin.restart_f64(mu, 0.1, 3, 99, chain0=2)
    wantr = np.array([[mu[i] + np.float32(0.1) * ora.langevin_normals_f32(i >> 2, 2 + c, 0, 99, ora.TAG_LANGEVIN_RESTART)[i & 3]
                       for i in range(9)] for c in range(3)], dtype=np.float32)
    np.testing.assert_allclose(r, wantr, rtol=0, atol=1e-6)


def test_chain_and_step_counters_wrap_as_uint32():
    rng = np.random.default_rng(3)
    d = 9
    x = rng.normal(size=(8, d)).astype(np.float32)
    k = rng.uniform(0.5, 2.0, size=d).astype(np.float32)
    mu = rng.normal(size=d).astype(np.float32)
    chain0, step0 = 2 ** 32 - 3, 2 ** 32 - 2
    np.testing.assert_array_equal(twin.wrap_ids(chain0, 8), np.array([2 ** 32 - 3, 2 ** 32 - 2, 2 ** 32 - 1, 0, 1, 2, 3, 4], np.uint32))
    # chains: all eight at once == chain by chain with the wrapped id
    whole, wt = twin.quadratic_f64(x, k, mu, 4, 0.02, 1.5, 0.7, 99, step0=7, chain0=chain0, trajectory=True)
    for c in range(8):
        one, ot = twin.quadratic_f64(x[c], k, mu, 4, 0.02, 1.5, 0.7, 99, step0=7, chain0=(chain0 + c) % 2 ** 32, trajectory=True)
        np.testing.assert_array_equal(one[0], whole[c])
        np.testing.assert_array_equal(ot[:, 0], wt[:, c])
    assert not np.array_equal(whole[3], twin.quadratic_f64(x[3], k, mu, 4, 0.02, 1.5, 0.7, 99, step0=7, chain0=3)[0])
    # steps: five at once == step by step with the wrapped counter
    whole, wt = twin.quadratic_f64(x, k, mu, 5, 0.02, 1.5, 0.7, 99, step0=step0, chain0=1, trajectory=True)
    cur = x
    for s in range(5):
        cur = twin.quadratic_f64(cur, k, mu, 1, 0.02, 1.5, 0.7, 99, step0=(step0 + s) % 2 ** 32, chain0=1)
        np.testing.assert_array_equal(cur, wt[s])
    np.testing.assert_array_equal(twin.quadratic_f64(wt[1], k, mu, 1, 0.02, 1.5, 0.7, 99, step0=0, chain0=1), wt[2])  # (2^32 - 2) + 2 = 0
    # both wraps at once against the oracle, whose counters are C uint32
    want, wtraj = ora.langevin_quadratic_f32(x, k, mu, 5, 0.02, 1.5, 0.7, 99, step0=step0, chain0=chain0, trajectory=True)
    got, traj = twin.quadratic_f64(x, k, mu, 5, 0.02, 1.5, 0.7, 99, step0=step0, chain0=chain0, trajectory=True)
    np.testing.assert_allclose(traj, wtraj, rtol=0, atol=1e-5)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)

"""K3 (csrc/langevin.hip): the routes and bookkeeping the small-shape parity tests do not reach.

A  the flat-grid variant of k3_langevin (n_chains > 65535: a 64-bit thread index split by t / quads, t % quads) and k3_restart,
   against the oracle and BIT FOR BIT against the 2-D variant (blockIdx.y = chain) run on the same chains in two smaller handles;
B  sample_from_energy with more than 65535 samples;
C  the coupled kernel on both sides of grid.y = 65535 and 65536 (8 chains per workgroup: 524280 / 524281 / 524289 chains);
D  the device's normals themselves against float64 Box-Muller on the same Philox words (tests/helpers/langevin_twin.py);
E  the uint32 wrap of chain0 + ch and step0 + s in every kernel;
F  one handle switched between energies with noise in the pad elements (pitch = dim rounded up to 4).
"""
import importlib.util
import os

import numpy as np
import pytest

from oracle import oracle as ora
from test_hip_parity import LANGEVIN_ATOL

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


twin = _load("langevin_twin")
mix = _load("mixture_twin")

COUPLED_TOL = 2e-4  # (1 + |x|): tests/test_langevin_coupled_gpu.py


def _mix_tol(d):  # tests/test_langevin_mixture_gpu.py
    return 2e-4 if d <= 64 else 1e-3


def _rows_equal(got, want, rows, what):
    """Named rows first (a failure says which side of a boundary broke), then everything."""
    for r in rows:
        assert np.array_equal(got[..., r, :], want[..., r, :]), f"{what}: chain {r} differs"
    np.testing.assert_array_equal(got, want, err_msg=what)


def _rows_close(got, want, rows, atol, what):
    for r in rows:
        err = float(np.max(np.abs(got[..., r, :].astype(np.float64) - want[..., r, :])))
        assert err <= atol, f"{what}: chain {r} is off by {err:.3g}"
    np.testing.assert_allclose(got, want, rtol=0, atol=atol, err_msg=what)


def _energy(dim, uni, seed):
    if uni:
        return 1.75, 0.25
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 2.0, size=dim).astype(np.float32), rng.normal(size=dim).astype(np.float32)


# ----------------------------------------------------------------------------- A: the flat-grid route
FLAT_SHAPES = [(65535, 5), (65536, 5), (65537, 12), (70001, 1)]  # last 2-D size; first flat size; t % quads no mask; one quad
STEP = dict(dt=0.02, gamma=1.5, T=0.7, seed=99)
CUT = 40000


def _run(hip, x, k, mu, n_steps, step0, chain0, spl=0):
    lc = hip.LangevinChains(x.shape[0], x.shape[1])
    lc.set_energy(k, mu)
    if spl:
        lc.set_kernel(steps_per_launch=spl)
    lc.set_state(x)
    traj = lc.step(n_steps, STEP["dt"], STEP["gamma"], STEP["T"], STEP["seed"], step0=step0, chain0=chain0, trajectory=True)
    got = lc.get_state()
    lc.close()
    return got, traj


@pytest.fixture(scope="module")
def hip():
    from tsu import _hip
    _hip.Context.default()
    return _hip


@pytest.mark.parametrize("uni", [False, True], ids=["general", "uniform"])
@pytest.mark.parametrize("n_chains,dim", FLAT_SHAPES)
def test_flat_route_matches_the_oracle_and_the_2d_route_bit_for_bit(hip, n_chains, dim, uni):
    x = np.random.default_rng(n_chains + dim).normal(size=(n_chains, dim)).astype(np.float32)
    k, mu = _energy(dim, uni, dim)
    got, traj = _run(hip, x, k, mu, 6, 3, 5)
    rows = [0, CUT - 1, CUT, 65534, n_chains - 1] + [r for r in (65535, 65536) if r < n_chains]
    # (b) the same chains on the 2-D route: two handles of at most 65535 chains, chain ids carried by chain0
    lo, tlo = _run(hip, x[:CUT], k, mu, 6, 3, 5)
    hi, thi = _run(hip, x[CUT:], k, mu, 6, 3, 5 + CUT)
    _rows_equal(got, np.concatenate([lo, hi]), rows, "state, one handle against two on the 2-D route")
    _rows_equal(traj, np.concatenate([tlo, thi], axis=1), rows, "trajectory, one handle against two on the 2-D route")
    np.testing.assert_array_equal(traj[-1], got)
    # (a) the oracle
    want, wtraj = ora.langevin_quadratic_f32(x, k, mu, 6, STEP["dt"], STEP["gamma"], STEP["T"], STEP["seed"], step0=3, chain0=5,
                                             trajectory=True)
    _rows_close(got, want, rows, LANGEVIN_ATOL, "state against the oracle")
    _rows_close(traj, wtraj, rows, LANGEVIN_ATOL, "trajectory against the oracle")


@pytest.mark.parametrize("uni", [False, True], ids=["general", "uniform"])
@pytest.mark.parametrize("n_chains,dim", [(65537, 12), (3, 1027)])
def test_split_launches_write_the_fused_trajectory(hip, n_chains, dim, uni):
    """(c) steps_per_launch = 4 on 6 steps: launches of 4 + 2, each writing its rows of the trajectory from its own step counter."""
    x = np.random.default_rng(dim).normal(size=(n_chains, dim)).astype(np.float32)
    k, mu = _energy(dim, uni, dim)
    fused, tf = _run(hip, x, k, mu, 6, 3, 5)
    split, ts = _run(hip, x, k, mu, 6, 3, 5, spl=4)
    rows = [0, n_chains - 1] + ([65535, 65536] if n_chains > 65536 else [])
    for s in range(6):
        _rows_equal(ts[s], tf[s], rows, f"trajectory row {s}, launches of 4 + 2 against one launch")
    _rows_equal(split, fused, rows, "state, launches of 4 + 2 against one launch")
    np.testing.assert_array_equal(ts[-1], split)
    assert not np.array_equal(tf[3], tf[4])


@pytest.mark.parametrize("n_chains,dim", [(65537, 12), (65536, 5)])
def test_restart_above_the_boundary(hip, n_chains, dim):
    """(d) k3_restart always takes the flat split: x_init + 0.1 N(0, 1) from the restart tag, chain ids from chain0 = 2."""
    x_init = np.random.default_rng(dim).normal(size=dim).astype(np.float32)
    lc = hip.LangevinChains(n_chains, dim)
    lc.restart(x_init, 0.1, 99, chain0=2)
    got = lc.get_state()
    lc.close()
    want = twin.restart_f64(x_init, 0.1, n_chains, 99, chain0=2)
    _rows_close(got, want, [0, 65535, n_chains - 1] + ([65536] if n_chains > 65536 else []), LANGEVIN_ATOL, "restart against the twin")
    # the same rows from a handle on the other side of the boundary, chain ids carried by chain0
    small = hip.LangevinChains(n_chains - CUT, dim)
    small.restart(x_init, 0.1, 99, chain0=2 + CUT)
    _rows_equal(got[CUT:], small.get_state(), [0, 65535 - CUT, n_chains - CUT - 1], "restart, chains from 40000 on in a handle of their own")
    small.close()


# ----------------------------------------------------------------------------- B: the public surface above the boundary
def test_sample_from_energy_with_more_than_65535_samples(hip):
    from tsu.core import QuadraticEnergy, ThermalSamplingUnit, TSUConfig
    n, seed = 66000, 42
    cfg = TSUConfig(temperature=0.7, dt=0.02, friction=1.5, n_burnin=2, n_steps=3)
    x_init = np.array([0.3, -1.2, 0.8])
    tsu = ThermalSamplingUnit(cfg, seed=seed)
    rows = [0, 1, 65534, 65535, 65536, n - 1]
    for call in range(2):  # the second call continues the chain ids: chain0 = 66000
        got = tsu.sample_from_energy(QuadraticEnergy(2.0, 0.5), x_init, n_samples=n)
        assert got.shape == (n, 3) and got.dtype == np.float64
        chain0 = call * n
        start = twin.restart_f64(x_init, 0.1, n, seed, chain0=chain0).astype(np.float32)
        start[0] = x_init.astype(np.float32)
        burnt = ora.langevin_quadratic_f32(start, 2.0, 0.5, cfg.n_burnin, cfg.dt, cfg.friction, cfg.temperature, seed, step0=0, chain0=chain0)
        want = ora.langevin_quadratic_f32(burnt, 2.0, 0.5, cfg.n_steps, cfg.dt, cfg.friction, cfg.temperature, seed, step0=cfg.n_burnin,
                                          chain0=chain0)
        _rows_close(got, want, rows, LANGEVIN_ATOL, f"call {call}")
    assert tsu.sample_count == 2 * n


# ----------------------------------------------------------------------------- C: the coupled kernel past grid.y = 65535
A4 = np.array([[2.0, 0.5, 0.0, 0.25], [0.5, 1.5, 0.5, 0.0], [0.0, 0.5, 1.0, 0.25], [0.25, 0.0, 0.25, 2.0]], np.float32)  # SPD
B4 = np.array([0.5, 0.0, -0.25, 1.0], np.float32)


@pytest.mark.parametrize("n_chains", [8 * 65535, 8 * 65535 + 1, 8 * 65536 + 1])
def test_coupled_kernel_on_both_sides_of_the_grid_limit(hip, n_chains):
    """8 chains per workgroup: 524280 chains are 65535 rows of workgroups, one more chain is a 65536th -- the last the device's
    reported maxGridSize (2147483647, 65536, 65536) names -- and 524289 chains a 65537th.  Two steps (the buffers change places
    once between them), the trajectory of the second."""
    x = np.random.default_rng(4).normal(size=(n_chains, 4)).astype(np.float32)
    lc = hip.LangevinChains(n_chains, 4)
    lc.set_coupling(A4, B4)
    lc.set_state(x)
    lc.step(1, 0.01, 1.0, 0.7, 99, step0=5, chain0=3)
    traj = lc.step(1, 0.01, 1.0, 0.7, 99, step0=6, chain0=3, trajectory=True)
    got = lc.get_state()
    lc.close()
    want = ora.langevin_coupled_f32(x, A4, B4, 2, 0.01, 1.0, 0.7, 99, step0=5, chain0=3)
    tol = COUPLED_TOL * (1.0 + np.abs(want))
    err = np.abs(got - want)
    for r in [0, 524279, 524280, 524287, 524288, n_chains - 1]:
        if r < n_chains:
            assert np.all(err[r] <= tol[r]), f"chain {r} is off by {float(err[r].max()):.3g} (got {got[r]}, want {want[r]})"
    assert np.all(err <= tol), (float(err.max()), int(np.argmax(err.max(axis=1))))
    np.testing.assert_array_equal(traj[0], got)


# ----------------------------------------------------------------------------- D: the normals against float64
def test_device_normals_against_float64_box_muller(hip):
    """One chain of 2^22 elements, k = 0, mu = 0, x = 0, T = 0.5, dt = gamma = 1: a = scale = 1 and the update
    fma(1, xi, fma(-0, 1, 0)) returns the device's normal exactly.  |xi| reaches 5.53 and the smallest u1 is 3 * 2^-24 here.

    The bound is 8 x the yardstick, the largest error of the oracle's float32 libm restatement against the same float64 twin,
    measured in the test (1.59e-6 where this was written: mostly the rounding of the angle 2 pi u2 to float32, which the device,
    working in revolutions, does not incur).  The device's native log2 / sqrt / sin / cos may be a few ulp where libm is under one.

    Measured on an MI355X: largest error of a normal 7.75e-7 (0.49 x the yardstick); radius part max |hypot(n0, n1) - r| = 8.1e-7,
    angle part max r |dtheta| = 4.0e-7 (largest |dtheta| 1.3e-7 rad)."""
    dim, seed, step0, chain0 = 1 << 22, 99, 3, 5
    lc = hip.LangevinChains(1, dim)
    lc.set_energy(0.0, 0.0)
    lc.set_state(np.zeros((1, dim), np.float32))
    lc.step(1, 1.0, 1.0, 0.5, seed, step0=step0, chain0=chain0)
    dev = lc.get_state()[0].astype(np.float64)
    lc.close()
    xi, r, ang = twin.normals_f64(np.arange(dim // 4, dtype=np.uint32), chain0, step0, twin.TAG_LANGEVIN, seed)
    xi = xi.reshape(-1)
    host = ora.langevin_quadratic_f32(np.zeros((1, dim), np.float32), 0.0, 0.0, 1, 1.0, 1.0, 0.5, seed, step0=step0, chain0=chain0)[0]
    yardstick = float(np.max(np.abs(host.astype(np.float64) - xi)))
    assert 2.0 ** -24 < yardstick < 4.5e-6, yardstick  # (float32 libm: see tests/test_langevin_twin_cpu.py)
    err = np.abs(dev - xi)
    n0, n1 = dev[0::2], dev[1::2]
    rr, aa = r.reshape(-1), ang.reshape(-1)
    e_rad = np.abs(np.hypot(n0, n1) - rr)
    dth = np.mod(np.arctan2(n1, n0) - aa + np.pi, 2.0 * np.pi) - np.pi
    e_ang = rr * np.abs(dth)  # (as a displacement of the pair, comparable with the other two)
    worst = int(np.argmax(err))
    msg = (f"device normals: max error {err.max():.3g} (element {worst}: {dev[worst]!r} for {xi[worst]!r}), radius part {e_rad.max():.3g}, "
           f"angle part {e_ang.max():.3g} (r |dtheta|; largest |dtheta| {np.abs(dth[rr > 0.1]).max():.3g} rad at r > 0.1); "
           f"yardstick (oracle float32 against float64) {yardstick:.3g}, bound {8 * yardstick:.3g}; max |xi| {np.abs(xi).max():.3f}")
    print(msg)
    assert np.all(np.isfinite(dev)), msg
    assert float(err.max()) <= 8.0 * yardstick, msg
    # tails: only an element within the bound of a threshold can change sides
    for thr in (3.0, 4.0):
        want_n, got_n = int(np.sum(np.abs(xi) > thr)), int(np.sum(np.abs(dev) > thr))
        assert want_n > 100 and abs(got_n - want_n) <= 2, (thr, got_n, want_n)
    assert float(np.abs(xi).max()) > 5.0 and float(np.abs(dev).max()) > 5.0


# ----------------------------------------------------------------------------- E: counter wrap
WRAP_CHAIN0, WRAP_STEP0 = 2 ** 32 - 3, 2 ** 32 - 2  # 8 chains: ids ..., 2^32 - 1, 0, ..., 4; 5 steps: ..., 2^32 - 1, 0, 1, 2


def _wrap_case(hip, dim, setup, reference, tol, relative=True):
    """8 chains, 5 steps across both wraps: against `reference` within tol (1 + |x|) (or tol alone), and bit for bit against a
    one-chain handle given each wrapped id."""
    x = (0.5 * np.random.default_rng(dim).normal(size=(8, dim))).astype(np.float32)
    lc = hip.LangevinChains(8, dim)
    setup(lc)
    lc.set_state(x)
    traj = lc.step(5, 0.01, 1.0, 0.7, 77, step0=WRAP_STEP0, chain0=WRAP_CHAIN0, trajectory=True)
    got = lc.get_state()
    lc.close()
    np.testing.assert_array_equal(traj[-1], got)
    want, wtraj = reference(x)
    assert np.all(np.abs(got - want) <= tol * (1.0 + np.abs(want) if relative else 1.0)), float(np.max(np.abs(got - want)))
    assert np.all(np.abs(traj - wtraj) <= tol * (1.0 + np.abs(wtraj) if relative else 1.0)), float(np.max(np.abs(traj - wtraj)))
    one = hip.LangevinChains(1, dim)
    setup(one)
    for c in range(8):
        one.set_state(x[c:c + 1])
        t1 = one.step(5, 0.01, 1.0, 0.7, 77, step0=WRAP_STEP0, chain0=(WRAP_CHAIN0 + c) % 2 ** 32, trajectory=True)
        assert np.array_equal(t1[:, 0], traj[:, c]), f"chain {c} (id {(WRAP_CHAIN0 + c) % 2 ** 32}) differs from a one-chain handle"
    # and step by step with the wrapped step counter
    one.set_state(x[3:4])
    for s in range(5):
        one.step(1, 0.01, 1.0, 0.7, 77, step0=(WRAP_STEP0 + s) % 2 ** 32, chain0=0)
        assert np.array_equal(one.get_state()[0], traj[s, 3]), f"step {s} (counter {(WRAP_STEP0 + s) % 2 ** 32}) differs"
    one.close()


@pytest.mark.parametrize("uni", [False, True], ids=["general", "uniform"])
def test_counters_wrap_in_the_separable_kernel(hip, uni):
    k, mu = _energy(9, uni, 9)
    _wrap_case(hip, 9, lambda lc: lc.set_energy(k, mu),
               lambda x: ora.langevin_quadratic_f32(x, k, mu, 5, 0.01, 1.0, 0.7, 77, step0=WRAP_STEP0, chain0=WRAP_CHAIN0, trajectory=True),
               LANGEVIN_ATOL, relative=False)
    lc = hip.LangevinChains(8, 9)
    # restart takes chain0 the same way
    lc.restart(mu, 0.1, 77, chain0=WRAP_CHAIN0)
    np.testing.assert_allclose(lc.get_state(), twin.restart_f64(np.broadcast_to(np.float32(mu), (9,)), 0.1, 8, 77, chain0=WRAP_CHAIN0),
                               rtol=0, atol=LANGEVIN_ATOL)
    lc.close()


def test_counters_wrap_in_the_coupled_kernel(hip):
    rng = np.random.default_rng(55)
    M = rng.normal(size=(5, 5))
    A = (M @ M.T / 5 + np.eye(5)).astype(np.float32)
    A = np.triu(A) + np.triu(A, 1).T
    b = rng.normal(size=5).astype(np.float32)
    _wrap_case(hip, 5, lambda lc: lc.set_coupling(A, b),
               lambda x: ora.langevin_coupled_f32(x, A, b, 5, 0.01, 1.0, 0.7, 77, step0=WRAP_STEP0, chain0=WRAP_CHAIN0, trajectory=True),
               COUPLED_TOL)


@pytest.mark.parametrize("dim", [10, 65])  # one lane per chain; one workgroup per chain
def test_counters_wrap_in_the_mixture_kernels(hip, dim):
    rng = np.random.default_rng(dim)
    c = (1.5 / np.sqrt(dim)) * rng.standard_normal((3, dim))
    w, sigma = np.array([1.0, 2.0, 0.5]), np.array([1.0, 0.8, 1.2])
    _wrap_case(hip, dim, lambda lc: lc.set_mixture(c, w, sigma, 1e-10),
               lambda x: mix.mixture_f32(x, c, w, sigma, 1e-10, 5, 0.01, 1.0, 0.7, 77, step0=WRAP_STEP0, chain0=WRAP_CHAIN0, trajectory=True),
               _mix_tol(dim))


# ----------------------------------------------------------------------------- F: one handle, several energies
@pytest.mark.parametrize("dim", [5, 65])  # three pad elements each; mixture: one lane / one workgroup per chain
def test_one_handle_switched_between_energies_with_noise_in_the_pad(hip, dim):
    """k3_restart and the separable kernel write noise into the elements between dim and the pitch; the mixture kernels mask them
    and the coupled kernel reads j < dim only: after any history a handle given an energy and a state is a fresh handle given
    the same, bit for bit -- also once an odd number of coupled steps has made the two state buffers change places."""
    n = 5
    rng = np.random.default_rng(dim)
    k, mu = _energy(dim, False, dim)
    c = (1.5 / np.sqrt(dim)) * rng.standard_normal((3, dim))
    w, sigma = np.array([1.0, 2.0, 0.5]), np.array([1.0, 0.8, 1.2])
    M = rng.normal(size=(dim, dim))
    A = (M @ M.T / dim + np.eye(dim)).astype(np.float32)
    A = np.triu(A) + np.triu(A, 1).T
    b = rng.normal(size=dim).astype(np.float32)
    x0 = (0.5 * rng.normal(size=(n, dim))).astype(np.float32)
    args = (0.01, 1.0, 0.7, 31)

    def fresh(setup, steps):
        lc = hip.LangevinChains(n, dim)
        setup(lc)
        lc.set_state(x0)
        t = lc.step(steps, *args, step0=2, chain0=1, trajectory=True)
        s = lc.get_state()
        lc.close()
        return s, t

    as_mixture = lambda lc: lc.set_mixture(c, w, sigma, 1e-10)  # noqa: E731
    as_coupled = lambda lc: lc.set_coupling(A, b)  # noqa: E731
    as_separable = lambda lc: lc.set_energy(k, mu)  # noqa: E731
    want = {name: fresh(setup, steps) for name, setup, steps in (("mixture", as_mixture, 8), ("coupled", as_coupled, 3),
                                                                 ("separable", as_separable, 8))}
    h = hip.LangevinChains(n, dim)

    def dirty():  # noise in every element of the current state buffer, pad included
        h.set_energy(k, mu)
        h.restart(mu, 1.0, 7, chain0=0)
        h.step(10, *args)

    def check(name, setup, steps, what):
        setup(h)
        h.set_state(x0)
        t = h.step(steps, *args, step0=2, chain0=1, trajectory=True)
        np.testing.assert_array_equal(t, want[name][1], err_msg=what + ": trajectory")
        np.testing.assert_array_equal(h.get_state(), want[name][0], err_msg=what + ": state")

    dirty()
    check("mixture", as_mixture, 8, "mixture after a separable run")
    dirty()
    check("coupled", as_coupled, 3, "coupled after a separable run")  # (three steps: the buffers have changed places)
    check("mixture", as_mixture, 8, "mixture on the other buffer")
    dirty()
    check("mixture", as_mixture, 8, "mixture on the other buffer after a separable run")
    dirty()
    check("coupled", as_coupled, 3, "coupled from the other buffer after a separable run")
    check("separable", as_separable, 8, "separable after a coupled run")
    h.close()

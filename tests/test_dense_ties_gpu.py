"""K2 dense kernels on forced near-ties (oracle.dense_tie_chain / dense_tie_bias), bit for bit, under every route.

Every dense kernel decides u < sigmoid(h / T) as x > logit(u) and lets the reference's float64 expression (gibbs.py:73-77,126)
decide near the logit and near the +-20 clamp.  Random draws almost never land there; these systems (couplings on a dyadic grid:
fields exact in any summation order) and draws put every decision there on purpose: inside the float64 band (A), between it and
the float band (B), just outside the float band (C), on the clamp ladder (D), at u in {0, 2^-53, 1 - 2^-53} (E) and where the
reference's rounded sigmoid and the exact comparison disagree (F).  Philox-mode cases craft the bias so that the first sweep of a
call lands every site near its own Philox uniform.  Each case compares the final state and every recorded state with the chain,
and asserts the route through launch_counts where it can."""
import os

import numpy as np
import pytest

from oracle import oracle as ora

pytestmark = pytest.mark.gpu

SEED = (1 << 33) + 977  # both key words matter
LADDER = 16
ANNEAL = [0.5, 0.7, 1.0, 0.5, 2.0, 0.25]
ANNEAL70 = [0.5 if k % 5 == 0 else (0.7, 1.0, 0.25, 2.0)[k % 4] for k in range(70)]


class _env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _system(n, seed, sym=True, ladder=True):
    J, b, _ = ora.dyadic_system(n, seed, sym=sym, ladder=min(LADDER, n) if ladder else 0,
                                rounding=max(0, min(LADDER, n - LADDER)) if ladder else 0)
    return J, b


def _dense(J, b, f64):
    from tsu import _hip
    return _hip.DenseSystem(J, b, _hip.DTYPE_F64 if f64 else _hip.DTYPE_F32)


def _chain(J, b, temps, seed, order=False, state=None):
    n = J.shape[0]
    rng = np.random.default_rng(seed)
    o = np.array([rng.permutation(n) for _ in temps]) if order else None
    ch = ora.dense_tie_chain(J, b, temps, order=o, rng=rng, state=state, ladder=min(LADDER, n))
    return o, ch


def _check_energies(d, J, b, states):
    """Where J and b share one grid and the sums stay below 2^53 units of it, energies are exact: no tolerance."""
    if not ora.energy_is_exact(J, b):
        return
    assert d.energy() == ora.c_dense_energy(d.get_state().astype(np.int64), J, b)
    np.testing.assert_array_equal(d.energies(states), [ora.c_dense_energy(s.astype(np.int64), J, b) for s in states])


def _replayed(d, J, b, seed, order=False, entry=("sweep", "sample", "anneal"), anneal=ANNEAL, route=None):
    """The replayed-uniform chains through sweep, sample and anneal, each from a fresh state."""
    n = J.shape[0]
    if "sweep" in entry:  # T = 0.5: the clamp ladder and the rounding sites are visited
        o, ch = _chain(J, b, [0.5] * 3, seed, order)
        d.set_state(ch["states"][0])
        d.sweep(0.5, 3, order=o, replay_uniforms=ch["uniforms"])
        np.testing.assert_array_equal(d.get_state(), ch["states"][-1])
        route and route()
    if "sample" in entry:  # burn-in 1, 2 samples of 2 sweeps, T = 0.7 (F / T is not F * (1 / T) exactly)
        o, ch = _chain(J, b, [0.7] * 5, seed + 1, order)
        d.set_state(ch["states"][0])
        got = d.sample(0.7, 1, 2, 2, order=o, replay_uniforms=ch["uniforms"])
        np.testing.assert_array_equal(got, ch["states"][[3, 5]])
        route and route()
    if "anneal" in entry:
        o, ch = _chain(J, b, anneal, seed + 2, order)
        d.set_state(ch["states"][0])
        got = d.anneal(anneal, order=o, replay_uniforms=ch["uniforms"])
        np.testing.assert_array_equal(got, ch["states"][1:])
        np.testing.assert_array_equal(d.get_state(), ch["states"][-1])
        route and route()
        _check_energies(d, J, b, ch["states"][1:])
    assert n == J.shape[0]


def _philox(J, T, seed, order=False, sweeps=2, f64=False, route=None, replica=3, sweep0=5, entry="sweep"):
    """Bias crafted for the first sweep of the call (non-dyadic: the device's bias-first sum may differ by an ulp), then ordinary
    sweeps; the fallback recomputes the Philox uniform from (site, sweep, replica tag, seed)."""
    n = J.shape[0]
    rng = np.random.default_rng(seed)
    s0 = rng.integers(0, 2, n).astype(np.int8)
    o = np.array([rng.permutation(n) for _ in range(sweeps)]) if order else None
    b, cls, s1 = ora.dense_tie_bias(J, T, None if o is None else o[0], SEED, sweep0, replica, s0, rng=rng)
    assert np.sum(cls != "R") >= 0.99 * n - 2
    d = _dense(J, b, f64)
    d.set_state(s0)
    if entry == "sweep":
        d.sweep(T, sweeps, seed=SEED, sweep0=sweep0, replica=replica, order=o)
        got = d.get_state()
    else:  # anneal at one temperature: the first recorded state is the crafted sweep
        rec = d.anneal([T] * sweeps, seed=SEED, sweep0=sweep0, replica=replica, order=o)
        np.testing.assert_array_equal(rec[0], s1)
        got = rec[-1]
    want = ora.dense_sweep_philox(s0, J, b, T, sweeps, SEED, sweep0=sweep0, replica=replica, order=o)
    np.testing.assert_array_equal(ora.dense_sweep_philox(s0, J, b, T, 1, SEED, sweep0=sweep0, replica=replica,
                                                         order=None if o is None else o[:1]), s1)
    np.testing.assert_array_equal(got, want)
    route and route(d)
    d.close()


def _no_own_no_pipe(d):
    assert d.launch_counts() == (0, 0)


# ------------------------------------------------------------------------------------------------ k2_small, k2_wg
@pytest.mark.parametrize("n,f64", [(1, False), (63, False), (64, False), (65, False), (128, False), (129, False), (192, False),
                                   (64, True), (128, True),  # k2_small, M = 1 / 2 / 3 slots
                                   (193, False), (528, False), (129, True), (448, True)])  # k2_wg
def test_one_wave_and_one_workgroup_kernels(n, f64):
    J, b = _system(n, 10 * n + f64, sym=n % 2 == 0)
    d = _dense(J, b, f64)

    def route():
        assert d.launch_counts() == (0, 0)
    _replayed(d, J, b, n, anneal=ANNEAL70 if n > 192 or f64 else ANNEAL, route=route)
    d.close()
    Jp, _ = _system(n, 10 * n + 5, sym=n % 2 == 1, ladder=False)
    _philox(Jp, 0.7, n, f64=f64, route=_no_own_no_pipe)
    # energies on the grid: a system without the ladder (its biases are off the grid)
    Je, be = _system(n, 10 * n + 7, ladder=False)
    d = _dense(Je, be, f64)
    _replayed(d, Je, be, n + 9, entry=("anneal",))
    d.close()


@pytest.mark.parametrize("n,R", [(64, 4), (192, 4), (193, 4), (528, 4)])
def test_replica_kernels(n, R):
    """k2_small_replicas (n <= 192) and k2_wg's replica launch: every replica is its own chain, its own uniforms and temperature;
    Philox mode: one state, one temperature, replica tags 0, 5, 6, 7 and the bias crafted for tag 5 (not the first)."""
    J, b = _system(n, 3 * n, sym=False)
    d = _dense(J, b, False)
    temps = [0.5, 0.7, 1.0, 0.25][:R]
    chains = [_chain(J, b, [T] * 2, 50 + r)[1] for r, T in enumerate(temps)]
    got = d.sweep_replicas(np.stack([c["states"][0] for c in chains]), temps, 2, [SEED] * R, [3] * R, list(range(R)),
                           replay_uniforms=np.stack([c["uniforms"] for c in chains]))
    np.testing.assert_array_equal(got, np.stack([c["states"][-1] for c in chains]))
    assert d.launch_counts() == (0, 0)
    d.close()
    _philox_replicas(n, R, own=False)


def _philox_replicas(n, R, own, f64=False):
    Jp, _ = _system(n, 3 * n + 1, ladder=False)
    rng = np.random.default_rng(n + R)
    s0 = rng.integers(0, 2, n).astype(np.int8)
    T, sweep0, tags = 0.7, 9, [0, 5, 6, 7, 9, 10, 11, 12][:R]
    b, cls, s1 = ora.dense_tie_bias(Jp, T, None, SEED, sweep0, tags[1], s0, rng=rng)
    d = _dense(Jp, b, f64)
    got = d.sweep_replicas(np.stack([s0] * R), [T] * R, 2, [SEED] * R, [sweep0] * R, tags)
    for r in range(R):
        np.testing.assert_array_equal(got[r], ora.dense_sweep_philox(s0, Jp, b, T, 2, SEED, sweep0=sweep0, replica=tags[r]), err_msg=str(r))
    if own:
        assert d.launch_counts()[0] >= 1
    d.close()


# ------------------------------------------------------------------------------------------------ k2_block
@pytest.mark.parametrize("n,f64", [(100, True), (300, False), (1000, False)])
def test_block_kernel_in_a_callers_order(n, f64):
    J, b = _system(n, 7 * n, sym=False)
    d = _dense(J, b, f64)

    def route():
        assert d.launch_counts() == (0, 0)
    _replayed(d, J, b, n, order=True, entry=("sweep", "sample"), route=route)
    d.close()
    Jp, _ = _system(n, 7 * n + 1, ladder=False)
    _philox(Jp, 0.7, n, order=True, f64=f64, route=_no_own_no_pipe)


# ------------------------------------------------------------------------------------------------ k2_pipe
def _pipe_route(d):
    own, pipe = d.launch_counts()
    assert own == 0 and pipe >= 1


@pytest.mark.parametrize("n,f64", [(580, False), (452, True), (4096, False)])
def test_pipeline_kernel(n, f64):
    """Natural order; from 2048 sites k2_own is made to give up at once so that the call runs on k2_pipe."""
    J, b = _system(n, 5 * n, sym=n != 580)
    with _env(TSU_K2_OWN_TEST_FAIL=0) if n >= 2048 else _env():
        d = _dense(J, b, f64)
        _replayed(d, J, b, n, entry=("sweep", "anneal"), route=lambda: _pipe_route(d))
        d.close()
        Jp, _ = _system(n, 5 * n + 1, sym=False, ladder=False)
        _philox(Jp, 0.5, n, f64=f64, route=_pipe_route)
        _philox(Jp, 0.7, n + 1, f64=f64, route=_pipe_route, entry="anneal", sweeps=3)


# ------------------------------------------------------------------------------------------------ k2_coop
@pytest.mark.parametrize("sweeps", [3, 70])
def test_cooperative_kernel_2051(sweeps):
    """2051 sites (not a multiple of 4: k2_own and k2_pipe decline) run on k2_coop, as test_dense_superblocks_match_oracle asserts."""
    n = 2051
    J, b = _system(n, 2051, sym=False)
    T = 0.5 if sweeps == 3 else 0.7
    o, ch = _chain(J, b, [T] * sweeps, sweeps)
    d = _dense(J, b, True)
    d.set_state(ch["states"][0])
    d.sweep(T, sweeps, replay_uniforms=ch["uniforms"])
    np.testing.assert_array_equal(d.get_state(), ch["states"][-1])
    assert d.launch_counts() == (0, 0)
    d.close()
    Jp, _ = _system(n, 2052, ladder=False)
    _philox(Jp, 0.7, sweeps, sweeps=sweeps, f64=sweeps == 3, route=_no_own_no_pipe)


# ------------------------------------------------------------------------------------------------ k2_own
def _own_route(d):
    assert d.launch_counts()[0] >= 1


@pytest.mark.parametrize("n,f64,order", [(2048, False, False), (4100, True, False), (2048, False, True)])
def test_owner_computes_kernel(n, f64, order):
    J, b = _system(n, 9 * n + order, sym=not order)
    d = _dense(J, b, f64)
    _replayed(d, J, b, n, order=order, entry=("sweep", "sample", "anneal") if order else ("sweep",), route=lambda: _own_route(d))
    d.close()
    Jp, _ = _system(n, 9 * n + 2, sym=False, ladder=False)
    _philox(Jp, 0.7, n, order=order, f64=f64, route=_own_route)
    if order:
        _philox(Jp, 0.5, n + 1, order=True, f64=f64, route=_own_route, entry="anneal", sweeps=2)


@pytest.mark.parametrize("n,R,f64", [(2304, 3, False), (4100, 8, True)])
def test_owner_computes_replicas(n, R, f64):
    J, b = _system(n, 4 * n + R, sym=False)
    temps = [0.5, 0.7, 1.0, 0.25, 0.5, 2.0, 0.7, 0.5][:R]
    chains = [_chain(J, b, [T] * 2, 70 + r)[1] for r, T in enumerate(temps)]
    d = _dense(J, b, f64)
    got = d.sweep_replicas(np.stack([c["states"][0] for c in chains]), temps, 2, [SEED] * R, [1] * R, list(range(1, R + 1)),
                           replay_uniforms=np.stack([c["uniforms"] for c in chains]))
    np.testing.assert_array_equal(got, np.stack([c["states"][-1] for c in chains]))
    assert d.launch_counts()[0] >= 1
    d.close()
    _philox_replicas(n, R, own=True, f64=f64)

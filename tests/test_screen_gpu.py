"""The fp32 screen of K7 / K8 on the GPU (screen() in csrc/disorder_dev.h), where the rest of the suite does not reach it:
a. the accuracy claimed for __expf and rcp, measured through tsu_probe_screen over the fp32 range (the table goes to
   profiles/screen_probe.txt);
b. decisions whose float64 threshold sits one margin outside the hi16 uniform's interval (screen_twin.edge_field: half of them
   screened, half decided exactly), end to end and bit for bit on single lattices, ladders and an ensemble;
c. disorder and temperatures past fp32 overflow (inf partial sums against the sign of the truth, c32 = inf, 0 * inf, c32 = 0).
tests/test_screen_cpu.py vets the inputs of b and c, so that none of this passes for want of a hard case."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import oracle as ora

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_spec = importlib.util.spec_from_file_location("screen_twin", os.path.join(HERE, "helpers", "screen_twin.py"))
st = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(st)

TS, SEED = st.TS, st.SEED


@pytest.fixture(scope="module")
def hip():
    from tsu import _hip
    return _hip


# ---------------------------------------------------------------- a. the instruction claim
def _probe_inputs():
    """Every 256th float32 bit pattern (2^24 values: every exponent, both signs, zeros, denormals, infinities, NaNs), the 4096
    floats on either side of 0, +-20, +-87.3, +-88.8 and +-104 (the clamp, where exp(-x) leaves the normal range, overflows, and
    where it has left every fp32), +-inf and NaN."""
    parts = [(np.arange(1 << 24, dtype=np.uint32) << np.uint32(8)).view(np.float32)]
    for c in (0.0, 20.0, 87.3, 88.8, 104.0):
        for sgn in (1.0, -1.0):
            b = np.array([sgn * c], np.float32).view(np.int32)[0] & 0x7FFFFFFF
            mag = np.arange(max(int(b) - 4096, 0), int(b) + 4097, dtype=np.uint32)
            parts.append((mag | np.uint32(0x80000000 if sgn < 0 else 0)).view(np.float32))
    parts.append(np.array([np.inf, -np.inf, np.nan], np.float32))
    return np.concatenate(parts)


def test_instruction_claim_through_the_probe(hip):
    """|t_dev - 2^16 sigma(x)| <= instr_bound(x) for every finite x (float64 reference, no clamp), m_dev = the twin's m32 bit for
    bit, t_dev NaN for a NaN x.  The largest |t_dev - ref| / instr_bound per decade of |x| is written to
    profiles/screen_probe.txt: the record of how far below its claim the hardware stays.  The case that refuted the claim's first
    form, (|x| + 2) u for __expf, is among the inputs and asserted by name: x = -44.994140625 errs by more than that form allows
    and by less than (1.23 |x| + 2) u."""
    x = _probe_inputs()
    t, m = hip.probe_screen(x, np.abs(x), np.float32(1.0))
    assert t.dtype == m.dtype == np.float32 and t.shape == m.shape == x.shape
    want_m = st.m32(np.abs(x), np.float32(1.0))
    assert (m.view(np.uint32) == want_m.view(np.uint32))[~np.isnan(x)].all(), "m differs from the twin's fused a32 |c32| + 4"
    assert np.isnan(m[np.isnan(x)]).all() and np.isnan(t[np.isnan(x)]).all()
    fin = np.isfinite(x)
    xf = x[fin].astype(np.float64)
    ref = 65536.0 * st.sigmoid64(xf)[0]
    err = np.abs(t[fin].astype(np.float64) - ref)
    bound = st.instr_bound(xf)
    ratio = err / bound
    assert (t[x == np.inf] == 65536.0).all() and (t[x == -np.inf] == 0.0).all()
    ax = np.abs(xf)
    edges = [0.0] + [10.0 ** k for k in range(-3, 2)] + [20.0, 40.0, 87.0, 100.0, np.inf]  # 87: where results begin to flush
    lines = ["# largest |t_dev - 2^16 sigma(x)| / instr_bound(x) per decade of |x| (tests/test_screen_gpu.py, tsu_probe_screen)",
             "# instr_bound = 2^16 u (p (1 - p) (1.23 |x| + 2) + 3 p) + 2^16 2^-126, u = 2^-24, p = sigma(x); x over every 256th",
             "# float32 bit pattern and the 4096 floats on either side of 0, +-20, +-87.3, +-88.8, +-104.  Rows are decades of |x|, 10 to 100",
             "# split at 20 (the clamp), 40 and 87 (beyond it exp(-x) or the reciprocal leaves the normal range and is flushed: the",
             "# ratio there is that of the flush term).  With (|x| + 2) in place of (1.23 |x| + 2) the 40 to 87 row exceeds 1.",
             "# |x| from         to       values   max ratio   at x"]
    for lo, hi in zip(edges[:-1], edges[1:]):
        sel = (ax >= lo) & (ax < hi)
        if sel.any():
            k = int(np.argmax(np.where(sel, ratio, -1.0)))
            lines.append(f"{lo:10.3g} {hi:10.3g} {int(sel.sum()):12d}   {ratio[k]:.4f}   {xf[k]:.9g}")
    k = int(np.argmax(ratio))
    lines.append(f"# overall: max ratio {ratio[k]:.4f} at x = {xf[k]:.9g} (t_dev {t[fin][k]:.9g}, reference {ref[k]:.9g})")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(os.path.join(ROOT, "profiles", "screen_probe.txt"), "w") as f:
        f.write(text)
    assert (err <= bound).all(), f"instruction claim exceeded {ratio[k]:.3f} times at x = {xf[k]!r}"
    i = int(np.flatnonzero(xf == -44.994140625)[0])
    p, q = st.sigmoid64(xf[i])
    first_form = 65536.0 * st.U * (p * q * (abs(xf[i]) + 2.0) + 3.0 * p) + 65536.0 * st.FLUSH
    assert first_form < err[i] <= bound[i], (err[i], first_form, bound[i])


def test_probe_takes_what_the_sweeps_take(hip):
    """Broadcast arguments, the three inputs independent, non-finite c32: against the twin (m bit for bit; t within the claim)."""
    rng = np.random.default_rng(5)
    f = rng.normal(size=(37, 53)).astype(np.float32) * 3
    a = (np.abs(f) + np.abs(rng.normal(size=f.shape))).astype(np.float32)
    for T in (0.4, 2.27, 5.0, 1e-30, 1e-39, 1e46):
        c = st.c32_of(T)
        t, m = hip.probe_screen(f, a, c)
        want_m, x = st.m32(a, c), st.x32(f, c)
        assert np.array_equal(m.view(np.uint32), want_m.view(np.uint32)), T
        ok = np.isfinite(x)
        assert np.isnan(t[np.isnan(x)]).all()
        xf = x[ok].astype(np.float64)
        assert (np.abs(t[ok] - 65536.0 * st.sigmoid64(xf)[0]) <= st.instr_bound(xf)).all(), T
    # a denormal c32 (T = 1e40) times a huge field is an ordinary x: the product must not lose the denormal factor
    c = st.c32_of(1e40)
    fb, ab = (f * np.float32(1e37)).astype(np.float32), (a * np.float32(1e37)).astype(np.float32)
    t, m = hip.probe_screen(fb, ab, c)
    xf = st.x32(fb, c).astype(np.float64)
    assert 0 < c < 2.0 ** -126 and np.abs(xf).max() > 1e-3
    assert np.array_equal(m.view(np.uint32), st.m32(ab, c).view(np.uint32))
    assert (np.abs(t - 65536.0 * st.sigmoid64(xf)[0]) <= st.instr_bound(xf)).all()
    with pytest.raises(ValueError):
        hip.probe_screen(np.zeros(0, np.float32), np.zeros(0, np.float32), np.float32(1.0))


# ---------------------------------------------------------------- b. decisions at the margin's edge
_cases = {}


def _edge(shape, periodic, scale, T, key, start_seed):
    """One case's (start, couplings, h), computed once; the input conditions are asserted again, they cost nothing here."""
    k = (shape, periodic, scale, T, key, start_seed)
    if k not in _cases:
        start = st.random_start(shape, start_seed, ora.ising2d_randomize)
        couplings, h, stats = st.edge_case(shape, periodic, scale, T, key, start)
        assert stats["band"] >= 0.95 and stats["screened"] >= 0.35 and stats["exact"] >= 0.35, stats
        _cases[k] = (start, couplings, h)
    return _cases[k]


def _lattice(hip, shape, periodic):
    return hip.Lattice(*shape, periodic) if len(shape) == 2 else hip.Lattice3D(*shape, periodic)


def _sweep(lat, T, n, seed, sweep0):
    (lat.disorder_sweep if lat.__class__.__name__ == "Lattice" else lat.sweep)(T, n, seed, sweep0, 0)


def _differ(got, want):
    return f"{int((got != want).sum())} sites differ, first {np.argwhere(got != want)[:4].tolist()}"


@pytest.mark.parametrize("T", st.TEMPS)
@pytest.mark.parametrize("scale", st.SCALES)
@pytest.mark.parametrize("shape,periodic", st.SHAPES_2D + st.SHAPES_3D)
def test_single_lattice_decisions_at_the_margins_edge(hip, shape, periodic, scale, T):
    """K7 Lattice.disorder_sweep and K8 Lattice3D.sweep: sweep 0 on the edge field, then two more, against the twin."""
    dim = len(shape)
    start, couplings, h = _edge(shape, periodic, scale, T, SEED, SEED + 1)
    lat = _lattice(hip, shape, periodic)
    try:
        lat.randomize(SEED + 1)
        assert (lat.get_spins() == start).all()
        lat.set_disorder(*couplings, h)
        want = start
        for sweep0, n in ((0, 1), (1, 2)):
            _sweep(lat, T, n, SEED, sweep0)
            want = st.sweep(dim, want, periodic, couplings, h, T, n, SEED, sweep0)
            got = lat.get_spins()
            assert (got == want).all(), f"sweep0 {sweep0}: " + _differ(got, want)
    finally:
        lat.close()


def _ladder(hip, shape, periodic):
    if len(shape) == 2:
        return hip.TemperingLattice(*shape, periodic, len(TS), 1)
    return hip.TemperingLattice3D(*shape, periodic, len(TS), 1)


@pytest.mark.parametrize("scale", st.SCALES)
@pytest.mark.parametrize("group", ["1", "3", "R"])
@pytest.mark.parametrize("shape,periodic", st.LADDER_SHAPES)
def test_ladder_decisions_at_the_margins_edge(hip, monkeypatch, shape, periodic, group, scale):
    """TemperingLattice / TemperingLattice3D with the field aimed at walker 3 (key seed + 3, T = 2.27): a wrong per-slot c32 or T
    moves its decisions off the twin's.  Walker 3 against the twin, every other walker against a standalone lattice."""
    dim, R, aim = len(shape), len(TS), 3
    monkeypatch.setenv("TSU_PT_GROUP", str(R) if group == "R" else group)
    start, couplings, h = _edge(shape, periodic, scale, TS[aim], SEED + aim, SEED + aim)
    pt = _ladder(hip, shape, periodic)
    lats = [_lattice(hip, shape, periodic) for _ in range(R)]
    try:
        pt.set_disorder(*couplings, h)
        pt.set_temperatures(TS)
        pt.init(SEED, 0)
        assert (pt.get_spins(0, aim) == start).all()
        for w, lat in enumerate(lats):
            lat.randomize(SEED + w)
            lat.set_disorder(*couplings, h)
        want = start
        for sweep0, n in ((0, 1), (1, 2)):
            pt.run(1, n, swap=False, record=False)
            want = st.sweep(dim, want, periodic, couplings, h, TS[aim], n, SEED + aim, sweep0)
            got = pt.get_spins(0, aim)
            assert (got == want).all(), f"walker {aim}, sweep0 {sweep0}: " + _differ(got, want)
            for w, lat in enumerate(lats):
                _sweep(lat, TS[w], n, SEED + w, sweep0)
                assert (pt.get_spins(0, w) == lat.get_spins()).all(), (w, sweep0)
    finally:
        pt.close()
        for lat in lats:
            lat.close()


@pytest.mark.parametrize("scale", st.SCALES)
def test_ensemble_decisions_at_the_margins_edge(hip, scale):
    """TemperingEnsemble, S = 3 on 37 x 53 open: the edge field sits in sample 1's disorder, aimed at its slot 2 (key 113 + 2,
    T = 1.5); samples 0 and 2 carry Gaussian disorder of their own.  The aimed walker against the twin, the fourteen others
    against standalone lattices."""
    shape, periodic, S, R, aim_s, aim_w = (37, 53), False, 3, len(TS), 1, 2
    seeds = [100, 113, 126]
    start, couplings, h = _edge(shape, periodic, scale, TS[aim_w], seeds[aim_s] + aim_w, seeds[aim_s] + aim_w)
    rng = np.random.default_rng(scale)
    dis = []
    for s in range(S):
        if s == aim_s:
            dis.append((couplings, h))
        else:
            dis.append((st.gaussian_couplings(shape, periodic, max(scale, 1), dseed=10 + s), rng.normal(size=shape).astype(np.float32)))
    ens = hip.TemperingEnsemble(*shape, periodic, S, R, 1)
    lats = [[hip.Lattice(*shape, periodic) for _ in range(R)] for _ in range(S)]
    try:
        ens.set_disorder(np.stack([d[0][0] for d in dis]), np.stack([d[0][1] for d in dis]), np.stack([d[1] for d in dis]))
        ens.set_temperatures(TS)
        ens.init(seeds, 0)
        assert (ens.get_spins(aim_s, 0, aim_w) == start).all()
        for s in range(S):
            for w, lat in enumerate(lats[s]):
                lat.randomize(seeds[s] + w)
                lat.set_disorder(*dis[s][0], dis[s][1])
        want = start
        for sweep0, n in ((0, 1), (1, 2)):
            ens.run(1, n, swap=False, record=False)
            want = st.sweep(2, want, periodic, couplings, h, TS[aim_w], n, seeds[aim_s] + aim_w, sweep0)
            got = ens.get_spins(aim_s, 0, aim_w)
            assert (got == want).all(), f"sweep0 {sweep0}: " + _differ(got, want)
            for s in range(S):
                for w, lat in enumerate(lats[s]):
                    lat.disorder_sweep(TS[w], n, seeds[s] + w, sweep0, 0)
                    assert (ens.get_spins(s, 0, w) == lat.get_spins()).all(), (s, w, sweep0)
    finally:
        ens.close()
        for row in lats:
            for lat in row:
                lat.close()


# ---------------------------------------------------------------- c. past overflow
def _energy_ok(dim, got, spins, periodic, couplings, h):
    want, terms = st.energy_terms(dim, spins, periodic, couplings, h)
    assert np.isfinite(got) and abs(got - want) <= 1e-12 * terms, (got, want, terms)


@pytest.mark.parametrize("T", st.HUGE_TS)
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape,periodic", st.HUGE_SHAPES[:2])
def test_single_lattices_past_overflow(hip, shape, periodic, sparse, T):
    """K7 16 x 40 and K8 (4, 6, 40) on huge disorder (all of it, or one value in ten) at T = 1 (inf partial sums), 1e-30 (A = inf),
    1e-39 (c32 = inf; no field and zero patches: 0 * inf) and 1e46 (c32 = 0): two sweeps against the twin, then the energy."""
    dim = len(shape)
    couplings, h = st.huge_case(shape, periodic, sparse, zero_field=(T == 1e-39))
    start = st.random_start(shape, 3, ora.ising2d_randomize)
    lat = _lattice(hip, shape, periodic)
    try:
        lat.randomize(3)
        lat.set_disorder(*couplings, h)
        _sweep(lat, T, 2, 7, 0)
        want = st.sweep(dim, start, periodic, couplings, h, T, 2, 7, 0)
        got = lat.get_spins()
        assert (got == want).all(), _differ(got, want)
        _energy_ok(dim, lat.disorder_energy() if dim == 2 else lat.energy(), want, periodic, couplings, h)
    finally:
        lat.close()


@pytest.mark.parametrize("zero_field", [False, True])
@pytest.mark.parametrize("sparse", [False, True])
def test_ladder_past_overflow(hip, sparse, zero_field):
    """A 2-D ladder, 16 x 40 open, whose four slots are the four temperatures: every walker against the twin after two sweeps,
    its energy against the twin's."""
    shape, periodic = st.HUGE_SHAPES[2]
    Ts = [1e-39, 1e-30, 1.0, 1e46]
    couplings, h = st.huge_case(shape, periodic, sparse, zero_field)
    pt = hip.TemperingLattice(*shape, periodic, len(Ts), 1)
    try:
        pt.set_disorder(*couplings, h)
        pt.set_temperatures(Ts)
        pt.init(40, 0)
        pt.run(1, 2, swap=False, record=False)
        E, _ = pt.energies()
        for w, T in enumerate(Ts):
            start = st.random_start(shape, 40 + w, ora.ising2d_randomize)
            want = st.sweep(2, start, periodic, couplings, h, T, 2, 40 + w, 0)
            got = pt.get_spins(0, w)
            assert (got == want).all(), f"walker {w} (T = {T}): " + _differ(got, want)
            _energy_ok(2, E[0, w], want, periodic, couplings, h)
    finally:
        pt.close()

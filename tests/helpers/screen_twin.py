"""The fp32 half of the K7 / K8 screen (csrc/disorder_dev.h: Octet::site, Octet::update, screen()), restated in NumPy.

fp32 add, multiply, fused multiply-add and compare are IEEE on the device and here, so everything the screen computes except
rcp(1 + __expf(-x)) is reproduced bit for bit: the fp32 field and sum of |terms| in the device's association order, x = f32 c32,
the margin m and the two comparisons.  What is left to the device, the accuracy of the two instructions, is stated by
instr_bound() and measured through tsu_probe_screen (tests/test_screen_gpu.py).

edge_field() is tie_field's sibling: it puts the float64 threshold of every decision of sweep 0 at about one margin from the
nearer end of the hi16 uniform's interval, where the screen decides for one half of the sites and hands the other half to the
exact branch.  huge_disorder() gives couplings whose fp32 partial sums overflow.
"""
import importlib.util
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


l3 = _load("lattice3d_twin")
thresholds = l3.thresholds

U = 2.0 ** -24          # half an ulp, relative: the unit of the comment above screen()
FLUSH = 2.0 ** -126     # the smallest normal fp32: v_exp_f32 and v_rcp_f32 flush what lies below
F32 = np.float32


# ---------------------------------------------------------------- the arithmetic of Octet and screen()
def _f32(seq):
    return [np.asarray(a, dtype=F32) for a in seq]


def field32(dim, J, s, h):
    """f32 of Octet::update.  J, s: the neighbours' couplings and spins in the order (z-1, z+1,) r-1, r+1, c-1, c+1 (dim 3 has
    the first two), a missing neighbour with J = 0; every addition is one fp32 operation, in the device's association."""
    J, s = _f32(J), _f32(s)
    assert len(J) == len(s) == 2 * dim and dim in (2, 3)
    h = np.asarray(h, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        if dim == 3:
            (Jb, Jf, Ju, Jd, Jl, Jr), (sb, sf, su, sd, sl, sr) = J, s
            f = (Jb * sb + Jf * sf) + Ju * su
        else:
            (Ju, Jd, Jl, Jr), (su, sd, sl, sr) = J, s
            f = Ju * su
        return ((((f + Jd * sd) + Jl * sl) + Jr * sr) + h).astype(F32)


def abs32(dim, J, h):
    """a32 of Octet::site: the fp32 sum of |terms| in the device's association."""
    J = [np.abs(a) for a in _f32(J)]
    assert len(J) == 2 * dim and dim in (2, 3)
    h = np.abs(np.asarray(h, dtype=F32))
    with np.errstate(over="ignore"):
        if dim == 3:
            Jb, Jf, Ju, Jd, Jl, Jr = J
            a = (Jb + Jf) + Ju
        else:
            Ju, Jd, Jl, Jr = J
            a = Ju
        return ((((a + Jd) + Jl) + Jr) + h).astype(F32)


def c32_of(T):
    """fl32(2 / T) as the host computes it: inf for a T below 2 / FLT_MAX, 0 for one above 2 / 2^-150."""
    with np.errstate(over="ignore", under="ignore"):
        return F32(2.0 / float(T))


def x32(f32, c32):
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return (np.asarray(f32, F32) * F32(c32)).astype(F32)


def A32(a32, c32):
    """A = a32 |c32| as screen() spells it (one fp32 product).  The device never holds this number: see m32."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return (np.asarray(a32, F32) * np.abs(F32(c32))).astype(F32)


def m32(a32, c32):
    """m = (A + 4) / 64 as the device computes it: the compiler contracts a32 |c32| + 4 into one fused multiply-add, so the sum is
    rounded once (the instruction is in the probe kernel and in both sweeps); the division by 64 is exact.  The exact fma is
    taken in float64: the product of two fp32 is exact there, the sum is rounded to odd (two-sum), then once to fp32."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        a = np.asarray(a32, F32).astype(np.float64)
        c = np.abs(np.asarray(c32, F32).astype(np.float64))
        p = a * c
        s = p + 4.0
        bb = s - p
        err = (p - (s - bb)) + (4.0 - bb)           # p + 4 = s + err exactly
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0.0)
        bits = np.ascontiguousarray(s).view(np.int64)  # s >= 4 > 0: the bit pattern orders as the value
        odd = np.where(err > 0.0, bits | 1, (bits - 1) | 1)
        s = np.where(fix, odd, bits).view(np.float64)
        return (s.astype(F32) * F32(1.0 / 64.0)).astype(F32)


def decide(t, m, hi):
    """screen()'s two comparisons in fp32: +1, -1 or 0 (decide exactly).  A NaN fails both."""
    t, m = np.asarray(t, F32), np.asarray(m, F32)
    h = np.asarray(hi).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        up = t >= (h + F32(1.0)) + m
        dn = t <= h - m
    return np.where(up, 1, np.where(dn, -1, 0)).astype(np.int8)


def sigmoid64(x):
    """sigma(x) and sigma(-x) in float64, neither losing its small end."""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore", under="ignore"):
        e = np.exp(-np.abs(x))
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    return np.where(x >= 0, big, small), np.where(x >= 0, small, big)


def t_ideal(x):
    """fp32(2^16 sigma(x)) with x taken as float64: the screen's t from instructions without error."""
    return (65536.0 * sigmoid64(x)[0]).astype(F32)


EXP_SLOPE = 1.23        # __expf's relative error per unit of |x|, in u: see instr_bound


def instr_bound(x):
    """What the comment above screen() claims for the two instructions, in hi16 units.  __expf(-x) is v_exp_f32 of
    fl(-x fl32(log2 e)): the constant is 0.23 u short of log2 e and the product rounds by u, which the exponential turns into
    1.23 |x| u relative; v_exp_f32 adds its 1 ulp <= 2 u.  That moves p = rcp(1 + e) by p (1 - p) (1.23 |x| + 2) u; the add and
    v_rcp_f32 (1 ulp) add 3 u p; 2^16 2^-126 for results the instructions flush.  (The comment first said (|x| + 2) u: the
    device exceeds that, by 1.097 at x = -44.994140625; test_screen_gpu.py keeps the case.)"""
    x = np.asarray(x, np.float64)
    p, q = sigmoid64(x)
    return 65536.0 * U * (p * q * (EXP_SLOPE * np.abs(x) + 2.0) + 3.0 * p) + 65536.0 * FLUSH


# ---------------------------------------------------------------- lattices: a 2-D lattice is the layer z = 0 of a 3-D one
def lift(dim, periodic, arrays):
    """(shape3, periodic3, arrays as (D, R, C)): a 2-D lattice becomes one open layer."""
    if dim == 3:
        return l3.axes(periodic), [np.asarray(a) for a in arrays]
    return (False, bool(periodic), bool(periodic)), [np.asarray(a)[None] for a in arrays]


def site_terms(dim, periodic, couplings, spins):
    """(J, s): per site the couplings (0 where the neighbour is missing) and spins of its 2 dim neighbours, in field32's order.
    couplings = (J_right, J_down[, J_layer]) of the lattice's shape."""
    per3, arr = lift(dim, periodic, list(couplings) + [spins])
    s = arr[-1].astype(F32)
    jr, jd = arr[0].astype(F32), arr[1].astype(F32)
    jl = arr[2].astype(F32) if dim == 3 else np.zeros_like(jr)
    idx = np.indices(s.shape)
    J, S = [], []
    for axis, Jx in ((0, jl), (1, jd), (2, jr)):
        if dim == 2 and axis == 0:
            continue
        n = s.shape[axis]
        has_prev = np.ones(s.shape, bool) if per3[axis] else idx[axis] > 0
        has_next = np.ones(s.shape, bool) if per3[axis] else idx[axis] < n - 1
        J.append(np.where(has_prev, np.roll(Jx, 1, axis=axis), F32(0)).astype(F32))
        S.append(np.roll(s, 1, axis=axis))
        J.append(np.where(has_next, Jx, F32(0)).astype(F32))
        S.append(np.roll(s, -1, axis=axis))
    if dim == 2:
        J, S = [a[0] for a in J], [a[0] for a in S]
    return J, S


def site_hi(dim, shape, hs, seed, replica=0):
    """The hi16 uniform of every site in half-sweep hs."""
    shape3 = tuple(shape) if dim == 3 else (1,) + tuple(shape)
    return (l3.site_uniforms(shape3, hs, seed, replica) >> np.uint32(16)).astype(np.int64).reshape(shape)


def field64(dim, periodic, couplings, h, spins):
    """The contract's float64 field of every site (lattice3d_twin.local_field; a 2-D lattice as one open layer)."""
    per3, arr = lift(dim, periodic, list(couplings) + [h, spins])
    jr, jd = arr[0].astype(F32), arr[1].astype(F32)
    jl = arr[2].astype(F32) if dim == 3 else np.zeros_like(jr)
    f = l3.local_field(arr[-1].astype(np.int8), per3, jr, jd, jl, arr[-2].astype(F32))
    return f if dim == 3 else f[0]


def screen_state(dim, periodic, couplings, h, spins, T):
    """Everything the screen sees at every site of a lattice in the state `spins`: dict of x32, m32, a32, f32, the float64 field
    f64 and thr16 = the contract's threshold / 2^16 (float64, exact: thr < 2^53)."""
    J, s = site_terms(dim, periodic, couplings, spins)
    c = c32_of(T)
    f, a = field32(dim, J, s, h), abs32(dim, J, h)
    f64 = field64(dim, periodic, couplings, h, spins)
    return {"f32": f, "a32": a, "x32": x32(f, c), "m32": m32(a, c), "f64": f64,
            "thr16": thresholds(f64, T).astype(np.float64) / 65536.0}


def half_sweep(dim, spins, periodic, couplings, h, T, hs, colour, seed, replica=0):
    """The contract's update of one colour (lattice3d_twin.half_sweep)."""
    per3, arr = lift(dim, periodic, list(couplings) + [h, spins])
    jr, jd = arr[0].astype(F32), arr[1].astype(F32)
    jl = arr[2].astype(F32) if dim == 3 else np.zeros_like(jr)
    out = l3.half_sweep(arr[-1].astype(np.int8), per3, jr, jd, jl, arr[-2].astype(F32), T, hs, colour, seed, replica)
    return out if dim == 3 else out[0]


def sweep(dim, spins, periodic, couplings, h, T, n_sweeps, seed, sweep0=0, replica=0):
    s = np.array(spins, dtype=np.int8)
    for k in range(int(n_sweeps)):
        for colour in (0, 1):
            s = half_sweep(dim, s, periodic, couplings, h, T, 2 * (int(sweep0) + k) + colour, colour, seed, replica)
    return s


def colours(shape):
    return np.indices(shape).sum(axis=0) & 1


# ---------------------------------------------------------------- decisions at the margin's edge
def _logit16(tau):
    """logit(tau / 65536) in float64, tau in (0, 65536)."""
    return np.log(tau) - np.log(65536.0 - tau)


def edge_field(shape, periodic, T, seed, replica, couplings, spins, spread=0.25, rounds=4, rng_seed=0):
    """(h, stats): an fp32 field that puts the float64 threshold of every decision of sweep 0, in units of 2^-16, at
    hi + 1 + m (1 + eps) or at hi - m (1 + eps): one margin, give or take `spread` of it, outside the interval [hi, hi + 1] of
    the site's own hi16 uniform, the side drawn per site (the other side where the drawn one leaves (0, 65536)), eps uniform in
    +-spread.  The target field is f = T / 2 logit(tau / 65536), h = fp32(f - neighbour sum); m depends on |h| through a32, so
    the fixed point is iterated `rounds` times.  Colour 0 is aimed in half-sweep 0 from the start state, colour 1 in half-sweep 1
    from the state the colour-0 half-sweep leaves (as tie_field does with couplings).

    stats: over all sites, each in its own half-sweep, 'band' = the share whose float64 thr / 2^16 lies between 0.75 m and
    1.25 m outside [hi, hi + 1]; 'screened' / 'exact' = the shares decide() settles / leaves to the exact branch with t from
    error-free instructions (t_ideal)."""
    dim = len(shape)
    shape = tuple(shape)
    rng = np.random.default_rng([int(rng_seed), int(seed) & 0xFFFFFFFF, dim])
    side = rng.random(shape) < 0.5
    eps = rng.uniform(-spread, spread, size=shape)
    col = colours(shape)
    c = c32_of(T)
    couplings = [np.asarray(a, F32).reshape(shape) for a in couplings]
    s = np.array(spins, dtype=np.int8).reshape(shape)
    h = np.zeros(shape, F32)
    band = np.zeros(shape, bool)
    dec = np.zeros(shape, np.int8)
    for colour in (0, 1):
        mine = col == colour
        hi = site_hi(dim, shape, colour, seed, replica).astype(np.float64)
        J, sn = site_terms(dim, periodic, couplings, s)
        nsum = field64(dim, periodic, couplings, np.zeros(shape, F32), s)
        hc = np.zeros(shape, F32)
        for _ in range(int(rounds)):
            m = m32(abs32(dim, J, hc), c).astype(np.float64)
            up, dn = hi + 1.0 + m * (1.0 + eps), hi - m * (1.0 + eps)
            tau = np.where(side, up, dn)
            tau = np.where(tau >= 65536.0, dn, np.where(tau <= 0.0, up, tau))
            tau = np.clip(tau, 2.0 ** -10, 65536.0 - 2.0 ** -10)
            hc = (0.5 * float(T) * _logit16(tau) - nsum).astype(F32)
        h = np.where(mine, hc, h).astype(F32)
        st = screen_state(dim, periodic, couplings, h, s, T)
        m = st["m32"].astype(np.float64)
        d = np.maximum(st["thr16"] - (hi + 1.0), hi - st["thr16"])  # > 0: outside [hi, hi + 1] by d
        band = np.where(mine, (d >= 0.75 * m) & (d <= 1.25 * m), band)
        dec = np.where(mine, decide(t_ideal(st["x32"]), st["m32"], hi), dec)
        if colour == 0:
            s = half_sweep(dim, s, periodic, couplings, h, T, 0, 0, seed, replica)
    n = float(band.size)
    return h, {"band": band.sum() / n, "screened": np.count_nonzero(dec) / n, "exact": np.count_nonzero(dec == 0) / n}


# ---------------------------------------------------------------- disorder past fp32 overflow
def huge_disorder(shape, rng, sparse=False):
    """fp32 values of a random sign and a magnitude uniform in [1e37, 3e38]: two of them of one sign overflow fp32.  sparse: O(1)
    Gaussian values with one in ten replaced by such a value."""
    big = (np.where(rng.random(shape) < 0.5, -1.0, 1.0) * rng.uniform(1e37, 3e38, size=shape)).astype(F32)
    if not sparse:
        return big
    return np.where(rng.random(shape) < 0.1, big, rng.normal(size=shape).astype(F32)).astype(F32)


def open_edges(dim, periodic, couplings):
    """The couplings with the last slice of every open axis set to 0, as set_disorder requires."""
    per3 = l3.axes(periodic) if dim == 3 else (False, bool(periodic), bool(periodic))
    out = [np.array(a, F32) for a in couplings]
    for k, axis in enumerate((-1, -2, -3)[:dim]):  # J_right: columns, J_down: rows, J_layer: layers
        if not per3[3 + axis]:
            out[k][(slice(None),) * (dim + axis) + (-1,)] = 0.0
    return out


def zero_patches(dim, periodic, couplings, h, rng, share=0.1):
    """One site in ten loses its field and every bond it has: its fp32 field and sum of |terms| are exactly 0, so c32 = inf
    meets 0 * inf there.  Returns new arrays."""
    couplings = [np.array(a, F32) for a in couplings]
    h = np.array(h, F32)
    z = rng.random(h.shape) < share
    h[z] = 0.0
    for k, axis in enumerate((-1, -2, -3)[:dim]):  # the bond to the next site along the axis, and the previous site's bond
        couplings[k][z | np.roll(z, -1, axis=axis)] = 0.0
    return couplings, h


# ---------------------------------------------------------------- the cases tests/test_screen_cpu.py vets and test_screen_gpu.py runs
TS = [0.4, 0.9, 1.5, 2.27, 5.0]
SCALES = (0, 1, 64)
TEMPS = (0.4, 2.27)
SHAPES_2D = [((64, 64), True), ((37, 53), False), ((128, 1000), True)]
SHAPES_3D = [((8, 6, 40), (False, True, True)), ((3, 5, 37), False), ((16, 16, 16), True)]
LADDER_SHAPES = [((64, 64), True), ((37, 53), False), ((8, 6, 40), (False, True, True))]
SEED = 13


def gaussian_couplings(shape, periodic, scale, dseed=0):
    """Gaussian couplings of standard deviation `scale` (0: none), the last slice of an open axis 0."""
    dim = len(shape)
    rng = np.random.default_rng([int(dseed), int(scale), dim] + list(shape))
    return open_edges(dim, periodic, [(rng.normal(size=shape) * scale).astype(F32) for _ in range(dim)])


def random_start(shape, seed, randomize):
    """The device's randomize(seed) of a lattice: randomize = oracle.ising2d_randomize (a 3-D lattice draws as its (D R) x C rows)."""
    rows = int(np.prod(shape[:-1]))
    return np.asarray(randomize(rows, shape[-1], int(seed)), np.int8).reshape(shape)


def edge_case(shape, periodic, scale, T, key_seed, start, dseed=0):
    """(couplings, h, stats) of one case: Gaussian couplings at `scale`, the edge field of the walker with Philox key key_seed
    (replica 0) at temperature T, starting from `start`."""
    couplings = gaussian_couplings(shape, periodic, scale, dseed)
    h, stats = edge_field(shape, periodic, T, key_seed, 0, couplings, start)
    return couplings, h, stats


HUGE_SHAPES = [((16, 40), True), ((4, 6, 40), (True, False, True)), ((16, 40), False)]  # K7, K8, the 2-D ladder
HUGE_TS = [1.0, 1e-30, 1e-39, 1e46]  # c32 = 2, 2e30 (A = inf), inf, 0


def huge_case(shape, periodic, sparse, zero_field=False):
    """The disorder of one past-overflow case: huge_disorder for every array, open edges.  zero_field: no field, and zero patches,
    so that c32 = inf meets 0 * inf."""
    dim = len(shape)
    rng = np.random.default_rng([dim, int(sparse)] + list(shape))
    arrays = [huge_disorder(shape, rng, sparse) for _ in range(dim + 1)]
    couplings, h = arrays[:dim], arrays[dim]
    if zero_field:
        couplings, _ = zero_patches(dim, periodic, couplings, h, rng)
        h = np.zeros(shape, F32)
    return open_edges(dim, periodic, couplings), h


def energy_terms(dim, spins, periodic, couplings, h):
    """(E, sum of |terms|) in float64 (lattice3d_twin.energy_terms; a 2-D lattice as one open layer)."""
    per3, arr = lift(dim, periodic, list(couplings) + [h, spins])
    jl = arr[2] if dim == 3 else np.zeros_like(arr[0])
    return l3.energy_terms(arr[-1], per3, arr[0], arr[1], jl, arr[-2])

"""The fp32 screen of K7 / K8 without a GPU (tests/helpers/screen_twin.py): the fp32 part of the error bound in the comment above
screen() holds on emulated sites with room for the instructions' claim; emulated decisions never contradict the contract; the
inputs of tests/test_screen_gpu.py do what they are for (decisions at the margin's edge, half of them screened; fp32 sums that
overflow against the sign of the truth); the twins' threshold against 50-digit arithmetic; the probe's restated lines, its header
and its ctypes prototype."""
import ctypes
import decimal
import functools
import importlib.util
import os
import re
import warnings

import numpy as np
import pytest

from oracle import oracle as ora

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_spec = importlib.util.spec_from_file_location("screen_twin", os.path.join(HERE, "helpers", "screen_twin.py"))
st = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(st)

NEW_SYMBOLS = ["tsu_probe_screen"]


# ---------------------------------------------------------------- sample sets: n = 4 (2-D) and n = 6 (3-D) additions
SET_SHAPES = {2: ((48, 48), True), 3: ((12, 12, 16), (True, False, True))}
SET_KINDS = [("gauss", s) for s in (0, 1, 8, 64, 512)] + [("pmJ", 1)]


@functools.lru_cache(maxsize=None)
def sample_set(dim, kind, scale, T):
    """Every site of a lattice in two states: the random start and the state after the colour-0 half-sweep.  Gaussian sets carry the
    field edge_field(spread=1) aims at the whole width of the margin (h cancels the neighbour sum: the sums' rounding weighs
    most there); the +-J set has no field.  Returns flat arrays x32, m32, thr16 and thr (uint64)."""
    shape, periodic = SET_SHAPES[dim]
    start = st.random_start(shape, 5 + dim, ora.ising2d_randomize)
    if kind == "gauss":
        couplings = st.gaussian_couplings(shape, periodic, scale, dseed=1)
        h, _ = st.edge_field(shape, periodic, T, 21, 0, couplings, start, spread=1.0)
    else:
        rng = np.random.default_rng(dim)
        couplings = st.open_edges(dim, periodic, [np.where(rng.random(shape) < 0.5, 1.0, -1.0).astype(np.float32) for _ in range(dim)])
        h = np.zeros(shape, np.float32)
    states = [start, st.half_sweep(dim, start, periodic, couplings, h, T, 0, 0, 21, 0)]
    out = {k: [] for k in ("x32", "m32", "thr16", "thr")}
    for s in states:
        ss = st.screen_state(dim, periodic, couplings, h, s, T)
        for k in ("x32", "m32", "thr16"):
            out[k].append(ss[k].ravel())
        out["thr"].append(st.thresholds(ss["f64"], T).ravel())
    return {k: np.concatenate(v) for k, v in out.items()}


@pytest.mark.parametrize("T", [0.4, 2.27])
@pytest.mark.parametrize("kind,scale", SET_KINDS)
@pytest.mark.parametrize("dim", [2, 3])
def test_fp32_arithmetic_leaves_room_for_the_instruction_claim(dim, kind, scale, T):
    """|2^16 sigma(x32) - thr / 2^16|, the error of everything in the screen but the two instructions, plus what instr_bound
    claims for those, plus 1 / 256 for the rounding of the comparisons' right-hand sides, stays within the margin at every site."""
    d = sample_set(dim, kind, scale, T)
    x = d["x32"].astype(np.float64)
    t_emul = np.abs(65536.0 * st.sigmoid64(x)[0] - d["thr16"])
    m = d["m32"].astype(np.float64)
    need = t_emul + st.instr_bound(x) + 1.0 / 256.0
    worst = int(np.argmax(need / m))
    print(f"dim {dim} {kind} scale {scale} T {T}: max T_emul / m = {np.max(t_emul / m):.4f}, max need / m = {need[worst] / m[worst]:.4f}")
    assert (need <= m).all(), (x[worst], t_emul[worst], need[worst], m[worst])
    if kind == "gauss":  # the set does what it is for: sites near p = 1/2, where a rounding of x moves t most
        assert np.mean(np.abs(x) < 2.0) > 0.1


@pytest.mark.parametrize("T", [0.4, 2.27])
@pytest.mark.parametrize("kind,scale", SET_KINDS)
@pytest.mark.parametrize("dim", [2, 3])
def test_emulated_decisions_never_contradict_the_contract(dim, kind, scale, T):
    """With t from error-free instructions, a screened decision is the contract's for every low half: +1 only if
    (hi, 65535) < thr, -1 only if (hi, 0) >= thr.  65536 random (site, hi) pairs, and per site the hi around t and around both
    ends of the margin."""
    d = sample_set(dim, kind, scale, T)
    t, m, thr = st.t_ideal(d["x32"]), d["m32"], d["thr"].astype(np.int64)
    rng = np.random.default_rng([dim, scale, int(T * 100)])
    idx = rng.integers(0, t.size, size=65536)
    groups = [(idx, rng.integers(0, 65536, size=65536))]
    allsites = np.arange(t.size)
    for centre in (t.astype(np.float64), t.astype(np.float64) - m, t.astype(np.float64) + m):
        for k in (-1, 0, 1):
            groups.append((allsites, np.clip(np.floor(centre) + k, 0, 65535).astype(np.int64)))
    seen = set()
    for i, hi in groups:
        dec = st.decide(t[i], m[i], hi)
        lo_u, hi_u = hi << 16, (hi << 16) | 65535
        assert (hi_u[dec > 0] < thr[i][dec > 0]).all()
        assert (lo_u[dec < 0] >= thr[i][dec < 0]).all()
        seen |= set(np.unique(dec).tolist())
    assert seen == {-1, 0, 1}


@pytest.mark.parametrize("dim", [2, 3])
def test_fp32_sums_err_by_n_u_S(dim):
    """The derivation's first step: with n = 2 dim fp32 additions, f32 and a32 lie within n u S of the float64 field and of
    S = the float64 sum of |terms|, every term counted, h included, when the terms cancel and when one dwarfs the rest."""
    rng = np.random.default_rng(dim)
    n, N = 2 * dim, 20000
    J = [(rng.normal(size=N) * 10.0 ** rng.integers(-3, 4, size=N)).astype(np.float32) for _ in range(n)]
    s = [np.where(rng.random(N) < 0.5, 1, -1).astype(np.int8) for _ in range(n)]
    f_nb = sum(j.astype(np.float64) * k for j, k in zip(J, s))
    h = np.where(rng.random(N) < 0.5, -f_nb * (1 + rng.normal(size=N) * 1e-3), rng.normal(size=N)).astype(np.float32)
    S = sum(np.abs(j.astype(np.float64)) for j in J) + np.abs(h.astype(np.float64))
    f64 = f_nb + h.astype(np.float64)
    assert (np.abs(st.field32(dim, J, s, h).astype(np.float64) - f64) <= n * st.U * S).all()
    a32 = st.abs32(dim, J, h).astype(np.float64)
    assert (np.abs(a32 - S) <= n * st.U * S).all()
    assert (a32 * (1 + n * st.U) >= np.abs(h)).all() and all((a32 * (1 + n * st.U) >= np.abs(j)).all() for j in J)


# ---------------------------------------------------------------- m32 is one rounding of a32 |c32| + 4
def test_m32_is_the_fused_sum_rounded_once():
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a = np.concatenate([np.abs(rng.normal(size=300)) * 10.0 ** rng.integers(-8, 8, size=300), [0.0, 2.0 ** -149, 3e38]]).astype(np.float32)
    c = np.concatenate([rng.uniform(0.1, 6.0, size=300), [5.0, 1.0, 0.88105726]]).astype(np.float32)
    got = st.m32(a, c)
    for ai, ci, gi in zip(a, c, got):
        exact = (Fraction(float(ai)) * Fraction(float(ci)) + 4) / 64
        lo, hi = np.nextafter(gi, np.float32(0)), np.nextafter(gi, np.float32(np.inf))
        assert abs(Fraction(float(gi)) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact)), (ai, ci)
    twice = ((a * c + np.float32(4.0)) * np.float32(1 / 64)).astype(np.float32)
    assert (twice != got).any()  # two roundings differ somewhere: the distinction is real
    assert st.m32(np.float32(np.inf), np.float32(1.0)) == np.inf and np.isnan(st.m32(np.float32(0.0), np.float32(np.inf)))


# ---------------------------------------------------------------- the inputs of the GPU tests
def _edge_cases():
    for shape, periodic in st.SHAPES_2D + st.SHAPES_3D:
        for scale in st.SCALES:
            for T in st.TEMPS:
                yield shape, periodic, scale, T, st.SEED, st.SEED + 1
    for shape, periodic in st.LADDER_SHAPES:       # ladders: aimed at walker 3 (key seed + 3, T = 2.27)
        for scale in st.SCALES:
            yield shape, periodic, scale, st.TS[3], st.SEED + 3, st.SEED + 3
    for scale in st.SCALES:                        # the ensemble: sample 1 (seed 113), slot 2
        yield (37, 53), False, scale, st.TS[2], 113 + 2, 113 + 2


@pytest.mark.parametrize("shape,periodic,scale,T,key,start_seed", list(_edge_cases()))
def test_edge_fields_sit_at_the_margins_edge(shape, periodic, scale, T, key, start_seed):
    """What test_screen_gpu.py relies on: >= 95 % of the sites have their float64 threshold between 0.75 m and 1.25 m outside
    [hi, hi + 1], and the emulation screens >= 35 % and sends >= 35 % to the exact branch."""
    start = st.random_start(shape, start_seed, ora.ising2d_randomize)
    _, h, stats = st.edge_case(shape, periodic, scale, T, key, start)
    print(shape, periodic, scale, T, stats)
    assert np.isfinite(h).all()
    assert stats["band"] >= 0.95, stats
    assert stats["screened"] >= 0.35 and stats["exact"] >= 0.35, stats


HUGE_SHAPES, HUGE_TS, huge_case = st.HUGE_SHAPES, st.HUGE_TS, st.huge_case


def _huge_sums(shape, periodic, sparse, zero_field):
    dim = len(shape)
    couplings, h = huge_case(shape, periodic, sparse, zero_field)
    start = st.random_start(shape, 3, ora.ising2d_randomize)
    J, s = st.site_terms(dim, periodic, couplings, start)
    return st.field32(dim, J, s, h), st.abs32(dim, J, h), st.field64(dim, periodic, couplings, h, start)


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape,periodic", HUGE_SHAPES)
def test_huge_disorder_overflows_against_the_sign_of_the_truth(shape, periodic, sparse):
    """The fp32 sum reaches +-inf while the float64 sum has the other sign, the sum of |terms| is inf wherever the fp32 sum is not
    finite, and the screen's numbers are then such that it cannot decide.  Share of sites with the wrong sign on dense huge
    disorder: >= 5 % with the seven terms of a 3-D site.  The five terms of a 2-D site reach it less often: two of them must
    overflow and the other three outweigh all; sampling the magnitudes huge_disorder draws gives 2.8 % (6.7 % for seven), so the
    two 2-D shapes, 640 sites each, are asked for 1 %, three standard deviations below that."""
    f32, a32, f64 = _huge_sums(shape, periodic, sparse, False)
    assert np.isfinite(f64).all() and not np.isnan(f32).any()
    bad = ~np.isfinite(f32)
    wrong = bad & (np.sign(f32) != np.sign(f64))
    print(shape, "sparse" if sparse else "dense", "non-finite", bad.mean(), "of the wrong sign", wrong.mean())
    assert np.isinf(a32[bad]).all() and bad.any()
    if not sparse:
        assert wrong.mean() >= (0.05 if len(shape) == 3 else 0.01)
    f0, a0, _ = _huge_sums(shape, periodic, sparse, True)
    assert (a0 == 0).mean() > 0.02 and (f0[a0 == 0] == 0).all()  # the zero patches: 0 * inf at c32 = inf
    for T in HUGE_TS:
        c = st.c32_of(T)
        for f, a in ((f32, a32), (f0, a0)):
            x, m = st.x32(f, c), st.m32(a, c)
            assert (st.decide(st.t_ideal(x), m, 12345)[~np.isfinite(m)] == 0).all()
            if T == 1e-39:
                assert np.isinf(c) and np.isnan(x[a == 0]).all() and np.isnan(m[a == 0]).all() and np.isinf(m[a > 0]).all()
            if T == 1e46:
                assert c == 0.0 and np.isnan(x[~np.isfinite(f)]).all() and (x[np.isfinite(f)] == 0).all()
            if T == 1e-30:
                assert np.isinf(m[a > 1e10]).all()


@pytest.mark.parametrize("T", HUGE_TS)
@pytest.mark.parametrize("shape,periodic", HUGE_SHAPES[:2])
def test_twins_run_clean_past_overflow(shape, periodic, T):
    """Two sweeps and the energy of the 2-D and 3-D twins on huge disorder with every warning an error."""
    dim = len(shape)
    start = st.random_start(shape, 3, ora.ising2d_randomize)
    for sparse in (False, True):
        couplings, h = huge_case(shape, periodic, sparse, zero_field=(T == 1e-39))
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            with np.errstate(all="raise"):
                out = st.sweep(dim, start, periodic, couplings, h, T, 2, 7)
                e, a = st.energy_terms(dim, out, periodic, couplings, h)
        assert set(np.unique(out).tolist()) <= {-1, 1} and np.isfinite(e) and np.isfinite(a)
        if T == 1e46:   # a temperature beyond every coupling: a coin per site
            assert 0.3 < (out > 0).mean() < 0.7


# ---------------------------------------------------------------- the twins' threshold against 50 digits
def test_twin_thresholds_against_decimal():
    """disorder_twin.thresholds against floor(sigma(x) 2^32 + 1/2) with sigma in 50-digit decimal arithmetic, clamped at +-20 as
    the contract has it: at most one unit of 2^-32 apart, and exactly 0 and 2^32 beyond the clamp."""
    rng = np.random.default_rng(0)
    edge = [np.nextafter(20.0, 0.0), 20.0, np.nextafter(20.0, 30.0), np.nextafter(-20.0, 0.0), -20.0, np.nextafter(-20.0, -30.0)]
    x = np.concatenate([rng.uniform(-22.0, 22.0, size=20000 - len(edge)), edge])
    got = st.thresholds(x, 2.0)  # f = x, T = 2: 2 f / T is x itself
    ctx = decimal.Context(prec=50)
    two32, half = decimal.Decimal(2 ** 32), decimal.Decimal("0.5")
    worst = 0
    for xi, gi in zip(x.tolist(), got.tolist()):
        if xi > 20.0:
            want = 2 ** 32
        elif xi < -20.0:
            want = 0
        else:
            p = ctx.divide(1, ctx.add(1, ctx.exp(ctx.minus(decimal.Decimal(xi)))))
            want = int(ctx.add(ctx.multiply(p, two32), half).to_integral_value(rounding=decimal.ROUND_FLOOR))
        if abs(xi) > 20.0:
            assert gi == want, xi
        worst = max(worst, abs(gi - want))
    assert worst <= 1, worst
    assert got[-1] == 0 and got[-4] == 2 ** 32 and got[-2] == got[-3] == 9 and got[-5] == got[-6] == 2 ** 32 - 9


# ---------------------------------------------------------------- the probe: restated lines, header, bindings
def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _norm(lines):
    return [re.sub(r"\s+", " ", ln).strip() for ln in lines]


def test_probe_restates_the_screens_four_lines():
    """probe.hip's probe_tm holds the four lines for x, A, t and m of screen()'s body, equal once whitespace is normalised, and
    nothing of the decision rule."""
    dev = _read("tsu-emulator_amd", "csrc", "disorder_dev.h")
    probe = _read("tsu-emulator_amd", "csrc", "probe.hip")
    body = re.search(r"\bint\s+screen\s*\([^)]*\)\s*\{(.*?)\n\}", dev, flags=re.S).group(1)
    mine = re.search(r"\bScreenTM\s+probe_tm\s*\([^)]*\)\s*\{(.*?)\n\}", probe, flags=re.S).group(1)
    head = _norm(body.strip().split("\n"))[:4]
    assert [ln.split("=")[0] for ln in head] == ["const float x ", "const float A ", "const float t ", "const float m "]
    assert _norm(mine.strip().split("\n"))[:4] == head
    assert _norm(mine.strip().split("\n"))[4:] == ["return {t, m};"]
    args = lambda text, name: re.sub(r"\s+", " ", re.search(name + r"\s*\(([^)]*)\)", text).group(1))
    assert args(dev, r"\bint\s+screen") == args(probe, r"\bScreenTM\s+probe_tm") + ", uint32_t hi"
    code = re.sub(r"//[^\n]*", "", probe)
    assert "exact_thr" not in code and not re.search(r"\bscreen\s*\(", code)


def test_header_and_ctypes_prototypes_agree():
    """The entry point is declared in include/tsu_hip_probe.h, which tsu_hip.h includes after tsu_hip_sparse_batch.h, exported by
    the library, and prototyped in _hip.PROBE_SIGNATURES (which load_library declares); the older sets are unchanged."""
    from tsu import _hip
    with open(os.path.join(ROOT, "include", "tsu_hip.h")) as f:
        top = f.read()
    assert re.search(r'^#include "tsu_hip_probe.h"', top, flags=re.M)
    assert top.index('#include "tsu_hip_sparse_batch.h"') < top.index('#include "tsu_hip_probe.h"')
    with open(os.path.join(ROOT, "include", "tsu_hip_probe.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tsu_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_hip.PROBE_SIGNATURES)
    lib = _hip.load_library()
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW_SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_hip.PROBE_SIGNATURES[name][1]), name
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == _hip.PROBE_SIGNATURES[name][1]
    older = (set(_hip.SIGNATURES) | set(_hip.CLUSTER3D_SIGNATURES) | set(_hip.CORRELATION_SIGNATURES) | set(_hip.POPULATION_SIGNATURES)
             | set(_hip.OVERLAP_SIGNATURES) | set(_hip.ENSEMBLE_SIGNATURES) | set(_hip.SPARSE_BATCH_SIGNATURES))
    assert not older & set(NEW_SYMBOLS)
    assert "tsu_hip_probe.h" in _read("tsu-emulator_amd", "csrc", "build.sh")
    assert callable(_hip.probe_screen)

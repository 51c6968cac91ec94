"""K11 on the host (no GPU needed): the library's acceptance table against the NumPy twin (tests/helpers/potts_muca_twin.py), the
twin's incremental bookkeeping against a recount, exact sampling of arbitrary weights against enumeration, the weight recursion with
a production run against the exact density of states, the refusals ahead of the device, and the new header with its ctypes
prototypes."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "tsu-emulator_amd", "csrc")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mt = _load("potts_muca_twin")

NEW_SYMBOLS = ("tsu_potts_muca_geometry", "tsu_potts_muca_thresholds", "tsu_potts_muca_create", "tsu_potts_muca_destroy",
               "tsu_potts_muca_set_weights", "tsu_potts_muca_set_spins", "tsu_potts_muca_get_spins", "tsu_potts_muca_fill",
               "tsu_potts_muca_set_tunnel_bounds", "tsu_potts_muca_run", "tsu_potts_muca_energies", "tsu_potts_muca_tunnels",
               "tsu_potts_muca_record", "tsu_potts_muca_clear_record", "tsu_potts_muca_measure", "tsu_potts_muca_route",
               "tsu_potts_muca_launch_count")

GEOMETRIES = [((1, 3, 3), False), ((1, 2, 2), (False, True, True)), ((1, 2, 6), (False, True, True)), ((1, 3, 5), (False, True, True)),
              ((1, 1, 7), False), ((1, 5, 1), (False, True, True)), ((2, 3, 4), (True, False, True)), ((2, 2, 2), True),
              ((1, 4, 4), (True, True, True)), ((3, 1, 1), (True, False, False)), ((1, 1, 1), True)]


def _id(case):
    shape, q, per = case[0], case[1], mt.axes(case[2])
    return "x".join(map(str, shape)) + f"-q{q}-" + "".join("p" if x else "o" for x in per)


def test_geometry_of_the_library_equals_the_twin():
    from tsu import _hip
    for shape, per in GEOMETRIES:
        assert _hip.potts_muca_geometry(*shape, per) == mt.geometry(shape, per), (shape, per)
    # open 2 x 3: 7 bonds; periodic 2 x 2: every bond doubled; a periodic ring of 5; a periodic axis of length 1 has no bond
    assert mt.geometry((1, 2, 3), False) == (7, 4) and mt.geometry((1, 2, 2), (False, True, True)) == (8, 4)
    assert mt.geometry((1, 1, 5), (False, False, True)) == (5, 4) and mt.geometry((1, 5, 1), (False, True, True)) == (5, 4)
    assert mt.geometry((2, 2, 2), False) == (12, 6) and mt.geometry((1, 4, 4), True) == (32, 6) and mt.geometry((1, 1, 1), True) == (0, 6)
    lib = _hip.load_library()
    per = np.zeros(3, np.int32)
    import ctypes as C
    b, z = C.c_int64(0), C.c_int(0)
    for shape in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (1, 256, 257), (65537, 1, 1), (2, 65536, 1)):
        assert lib.tsu_potts_muca_geometry(*shape, _hip._ptr(per, _hip._i32p), C.byref(b), C.byref(z)) == _hip.TSU_E_INVALID, shape
    assert _hip.potts_muca_geometry(1, 256, 256, False) == (2 * 256 * 255, 4)


def test_table_of_the_library_equals_the_twin():
    """Byte for byte on random ln W, with ties (always accept), steep drops (thr = 0) and both table widths."""
    from tsu import _hip
    rng = np.random.default_rng(5)
    seen_tie = seen_zero = seen_mid = 0
    for shape, per in GEOMETRIES:
        B, zmax = mt.geometry(shape, per)
        for kind in range(3):
            lnw = rng.normal(size=B + 1) * (1.0, 8.0, 40.0)[kind]
            if B >= 3:
                lnw[rng.integers(0, B + 1, size=(B + 1) // 3)] = lnw[0]  # ties
                lnw[rng.integers(0, B + 1)] = -60.0                      # a level no move reaches
            got = _hip.potts_muca_thresholds(B, zmax, lnw)
            want = mt.thresholds(B, zmax, lnw)
            assert got.shape == want.shape == (B + 1, 2 * zmax + 1) and got.tobytes() == want.tobytes(), (shape, per, kind)
            n, d = np.meshgrid(np.arange(B + 1), np.arange(-zmax, zmax + 1), indexing="ij")
            inside = (n + d >= 0) & (n + d <= B)
            assert (got[~inside] == 0).all() and (got[inside & (d == 0)] == 2 ** 32).all() and int(got.max()) <= 2 ** 32
            seen_tie += int(np.count_nonzero(got[inside & (d != 0)] == 2 ** 32))
            seen_zero += int(np.count_nonzero(got[inside] == 0))
            seen_mid += int(np.count_nonzero((got[inside] > 0) & (got[inside] < 2 ** 32)))
    assert seen_tie > 100 and seen_zero > 100 and seen_mid > 100
    # the edges of the rule: a drop too small for float64 to see is still a tie-free 2^32 - ... floor; 2^-32 is the last non-zero
    t = _hip.potts_muca_thresholds(1, 4, [0.0, -32 * math.log(2.0)])
    assert int(t[0, 5]) == int(math.floor(math.exp(-32 * math.log(2.0)) * 4294967296.0)) and int(t[1, 3]) == 2 ** 32
    assert int(_hip.potts_muca_thresholds(1, 4, [0.0, -23.0])[0, 5]) == 0
    for bad in ([0.0, float("nan")], [float("inf"), 0.0]):
        with pytest.raises(ValueError):
            _hip.potts_muca_thresholds(1, 4, bad)
    with pytest.raises(ValueError):
        _hip.potts_muca_thresholds(1, 5, [0.0, 0.0])


@pytest.mark.parametrize("case", [((1, 3, 3), 3, False), ((1, 2, 2), 4, (False, True, True)), ((1, 3, 5), 8, (False, True, True)),
                                  ((2, 3, 4), 2, (True, False, True)), ((1, 5, 1), 3, (False, True, True)), ((1, 1, 7), 5, False)], ids=_id)
def test_incremental_bookkeeping_equals_a_recount(case):
    shape, q, per = case
    rng = np.random.default_rng(6)
    B, _ = mt.geometry(shape, per)
    s = rng.integers(0, q, size=(37,) + shape).astype(np.int8)
    lnw = 0.2 * np.arange(B + 1) + rng.normal(size=B + 1)
    out = mt.run(s, q, per, lnw, 5, 2 ** 64 - 3, sweep0=2 ** 32 - 2, replica=3, bounds=(B // 3, B - B // 3) if B >= 3 else None)
    n, N = mt.count(out["spins"], q, per)
    assert (out["n"] == n).all() and (out["N"] == N).all() and (N.sum(axis=1) == np.prod(shape)).all()
    assert int(out["H"].sum()) == 37 * 5 and (out["spins"] != s).any()
    assert out["spins"].min() >= 0 and out["spins"].max() < q
    # a run split in two equals one run: state, record and tunnel state carried over
    a = mt.run(s, q, per, lnw, 2, 2 ** 64 - 3, sweep0=2 ** 32 - 2, replica=3, bounds=(B // 3, B - B // 3) if B >= 3 else None)
    b = mt.run(a["spins"], q, per, lnw, 3, 2 ** 64 - 3, sweep0=0, replica=3, record=a, side=a["side"], tunnels=a["tunnels"],
               bounds=(B // 3, B - B // 3) if B >= 3 else None)
    for k in ("spins", "n", "H", "S1", "S2", "side", "tunnels"):
        assert (b[k] == out[k]).all(), k


def test_proposal_is_never_the_current_colour_and_uniform_over_the_others():
    P = np.random.default_rng(1).integers(0, 2 ** 32, size=200000, dtype=np.uint64)
    P[:4] = (0, 2 ** 32 - 1, 2 ** 31, 2 ** 31 - 1)
    for q in range(2, 9):
        for c in range(q):
            cn = (c + 1 + ((P * np.uint64(q - 1)) >> np.uint64(32)).astype(np.int64)) % q
            assert (cn != c).all() and cn.min() >= 0 and cn.max() < q
            counts = np.bincount(cn, minlength=q)[[x for x in range(q) if x != c]]
            assert abs(counts / len(P) - 1.0 / (q - 1)).max() < 6 * np.sqrt(0.25 / len(P))


@pytest.mark.parametrize("case", mt.CHI2_CASES, ids=_id)
def test_twin_samples_arbitrary_weights_exactly(case):
    """The final states of 16384 independent walkers after 200 sweeps from the all-0 state against W(n_eq(s)) / sum over all q^N
    states, ln W[n] = 0.3 n + 0.7 normal(seed); cells with expected count >= 5 one each, the rest pooled.  The twin gives (the
    device equals it bit for bit, so the first line is the GPU test's number too):
      open 2x3 q=3:                 chi2 = 703.4 on 728 dof, p = 0.737, pooled 0 %
      open 3x3 q=2:                 chi2 = 505.2 on 510 dof, p = 0.551, pooled 0.06 %
      periodic 2x2 q=4:             chi2 = 266.3 on 255 dof, p = 0.301, pooled 0 %
      open 2x2x2 q=2:               chi2 = 223.6 on 240 dof, p = 0.769, pooled 0.21 %
      1x5 periodic ring q=3:        chi2 = 232.6 on 242 dof, p = 0.656, pooled 0 %"""
    shape, q, per, wseed, seed = case
    lnw = mt.chi2_weights(shape, per, wseed)
    out = mt.run(np.zeros((mt.CHI2_WALKERS,) + shape, np.int8), q, per, lnw, mt.CHI2_SWEEPS, seed)
    chi2, dof, p, pooled = mt.weight_chi2(mt.codes(out["spins"], q), shape, q, per, lnw)
    print(f"\n{_id(case)}: chi2 = {chi2:.1f} on {dof} dof, p = {p:.3f}, pooled {100 * pooled:.2f} %")
    assert p >= 0.01 and pooled <= 0.05


END_TO_END = [((1, 3, 3), 3, False, 7000), ((1, 2, 4), 4, (False, False, True), 7001)]


@pytest.mark.parametrize("case", END_TO_END, ids=_id)
def test_recursion_and_production_against_the_exact_density_of_states(case):
    """4096 walkers, 8 iterations of 20 sweeps from ln W = 0 (the package's own recursion on the twin's histograms), then 100
    production sweeps with the weights fixed.  Every level with g > 0 is visited and no other; max |ln g_hat - ln g_exact| <= 0.1;
    the reweighted <n_eq>, <N_max> and <N_max^2> at T = 0.5, 0.9, 1.5, 3.0 lie within 1 % of enumeration.  The twin gives:
      open 3x3 q=3:             max |d ln g| = 0.013, averages within 0.14 %
      2x4 q=4, periodic columns: max |d ln g| = 0.019, averages within 0.30 %"""
    from tsu.models import potts_muca as pm
    shape, q, per, seed = case
    B, _ = mt.geometry(shape, per)
    sites = int(np.prod(shape))
    lnw = np.zeros(B + 1)
    s = np.zeros((4096,) + shape, np.int8)
    t = 0
    for _ in range(8):
        out = mt.run(s, q, per, lnw, 20, seed, sweep0=t)
        s, t = out["spins"], t + 20
        lnw = pm.muca_recursion(lnw, out["H"])
        assert lnw.max() == 0.0
    out = mt.run(s, q, per, lnw, 100, seed, sweep0=t)
    n_all, nmax_all = mt.enumerate_states(shape, q, per)
    g = np.bincount(n_all, minlength=B + 1)
    assert ((out["H"] > 0) == (g > 0)).all() and int(out["H"].sum()) == 4096 * 100
    ln_g = pm.muca_density_of_states(out["H"], lnw, q, sites)
    err = float(np.abs(ln_g[g > 0] - np.log(g[g > 0])).max())
    assert np.isneginf(ln_g[g == 0]).all()
    res = pm.muca_reweight(out["H"], out["S1"], out["S2"], lnw, [0.5, 0.9, 1.5, 3.0], 1.0, q, sites)
    worst = 0.0
    for k, T in enumerate(res["temperatures"]):
        w = np.exp((n_all - n_all.max()) / T)
        w /= w.sum()
        for key, exact in (("n_eq", w @ n_all), ("n_max", w @ nmax_all), ("n_max2", w @ (nmax_all.astype(np.float64) ** 2))):
            worst = max(worst, abs(res[key][k] / exact - 1.0))
        assert abs(res["energy"][k] + (w @ n_all) / sites) <= 0.01 * (w @ n_all) / sites
    print(f"\n{_id(case)}: max |d ln g| = {err:.3f}, averages within {100 * worst:.2f} %")
    assert err <= 0.1 and worst <= 0.01


def test_reweighting_an_exact_record_gives_the_canonical_averages():
    """With H = g W exactly (the record an infinite flat run would leave) the reweighted averages are the enumeration's, for either
    sign of the coupling, and the density of states comes back normalised to q^N."""
    from tsu.models import potts_muca as pm
    shape, q, per = (1, 2, 3), 3, False
    n_all, nmax_all = mt.enumerate_states(shape, q, per)
    B = 7
    g = np.bincount(n_all, minlength=B + 1).astype(np.float64)
    lnw = -np.log(np.where(g > 0, g, 1.0)) + 3.0
    H = np.where(g > 0, 1000.0, 0.0)  # g W up to a constant
    S1 = np.array([1000.0 * nmax_all[n_all == n].mean() if g[n] else 0.0 for n in range(B + 1)])
    S2 = np.array([1000.0 * (nmax_all[n_all == n].astype(np.float64) ** 2).mean() if g[n] else 0.0 for n in range(B + 1)])
    ln_g = pm.muca_density_of_states(H, lnw, q, 6)
    assert np.allclose(np.exp(ln_g[g > 0]), g[g > 0]) and abs(np.exp(ln_g[g > 0]).sum() - 3 ** 6) < 1e-6
    for J in (1.0, -0.7):
        res = pm.muca_reweight(H, S1, S2, lnw, [0.6, 2.0], J, q, 6)
        for k, T in enumerate((0.6, 2.0)):
            w = np.exp(J * n_all / T)
            w /= w.sum()
            e = -J * n_all / 6
            m = (q * nmax_all / 6 - 1.0) / (q - 1.0)
            assert np.isclose(res["energy"][k], w @ e) and np.isclose(res["specific_heat"][k], 6 * (w @ e ** 2 - (w @ e) ** 2) / T ** 2)
            assert np.isclose(res["order_parameter"][k], w @ m) and np.isclose(res["susceptibility"][k], 6 * (w @ m ** 2 - (w @ m) ** 2) / T)
    # the recursion: linear continuation outside the visited range with the least-squares slope of its outermost bins (here all
    # three visited ones, at either end), holes inside it untouched, maximum at 0; the slope is capped
    new = pm.muca_recursion(np.array([5.0, 1.0, 2.0, 3.0, 4.0, 9.0]), np.array([0, 10, 0, 100, 10, 0]))
    a, b, c = 1.0 - np.log(10), 3.0 - np.log(100), 4.0 - np.log(10)
    x = np.array([1.0, 3.0, 4.0])
    slope = ((x - x.mean()) * (np.array([a, b, c]) - (a + b + c) / 3)).sum() / ((x - x.mean()) ** 2).sum()
    want = np.array([a - slope, a, 2.0, b, c, c + slope])
    assert np.allclose(new, want - want.max()) and abs(slope) < pm.MUCA_EDGE_SLOPE
    steep = pm.muca_recursion(np.zeros(6), np.array([0, 0, 1, 10 ** 9, 0, 0]))
    assert np.allclose(np.diff(steep), [-4.0, -4.0, -np.log(1e9), -4.0, -4.0]) and steep.max() == 0.0
    lone = pm.muca_recursion(np.zeros(4), np.array([0, 7, 0, 0]))
    assert np.allclose(lone, 0.0)
    assert pm.muca_flatness([0, 10, 0, 100, 10, 0]) == (1, 4, 0.25, 1)
    assert pm.muca_flatness([0, 30, 60, 30]) == (1, 3, 0.75, 0) and pm.muca_flatness([0, 0]) == (0, -1, 0.0, 0)
    with pytest.raises(ValueError):
        pm.muca_density_of_states(np.zeros(4), np.zeros(4), 3, 4)


def test_refusals_come_before_the_device(monkeypatch):
    import tsu
    from tsu import _hip
    from tsu.models import potts_muca

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_hip.Context, "default", classmethod(no_device))
    monkeypatch.setattr(_hip, "PottsMucaWalkers", no_device)
    bad = [dict(q=1), dict(q=9), dict(q=2.5), dict(q=True), dict(size=0), dict(size=(4, 0)), dict(size=(4, 4, 4, 4)), dict(size=(4,)),
           dict(size=(256, 257)), dict(size=(41, 40, 40)), dict(walkers=0), dict(walkers=2 ** 20 + 1), dict(walkers=2.5),
           dict(size=(256, 256), walkers=2 ** 15), dict(coupling=float("nan")), dict(coupling=float("inf")),
           dict(periodic=(True, True, True)), dict(size=(4, 4, 4), periodic=(True, True)), dict(periodic="yes")]
    for kw in bad:
        args = dict(size=4, q=3, walkers=64)
        args.update(kw)
        with pytest.raises(tsu.ConfigurationError):
            tsu.PottsMulticanonical(**args)
    # odd periodic sides, a periodic axis of length 1, the largest lattice and the largest population reach the handle
    for kw in (dict(size=(3, 5)), dict(size=(1, 7)), dict(size=(5, 1)), dict(size=(2, 3, 4), periodic=(True, False, True)),
               dict(size=(256, 256), walkers=2 ** 15 - 1), dict(size=(1, 2), walkers=2 ** 20), dict(coupling=-1.0), dict(q=8)):
        args = dict(size=4, q=3, walkers=64)
        args.update(kw)
        with pytest.raises(AssertionError, match="device was touched"):
            tsu.PottsMulticanonical(**args)
    for kw in (dict(temperatures=[1.0, -1.0]), dict(temperatures=[float("nan")]), dict(temperatures=[1.0], q=9),
               dict(temperatures=[1.0], walkers=0)):
        args = dict(size=4, q=3)
        args.update(kw)
        with pytest.raises(tsu.ConfigurationError):
            potts_muca.potts_multicanonical_scan(**args)
    with pytest.raises(ValueError):
        potts_muca.potts_multicanonical_scan(4, 3, [1.0], n_production=0)
    with pytest.raises(AssertionError, match="device was touched"):
        potts_muca.potts_multicanonical_scan(4, 3, [1.0])


def test_header_symbols_and_prototypes():
    from tsu import _hip
    with open(os.path.join(ROOT, "include", "tsu_hip.h")) as f:
        top = f.read()
    assert re.search(r'^#include "tsu_hip_potts_muca.h"', top, flags=re.M)
    assert top.index('#include "tsu_hip_potts3d.h"') < top.index('#include "tsu_hip_potts_muca.h"')
    assert not any(re.search(r"\b" + n + r"\s*\(", re.sub(r"/\*.*?\*/", "", top, flags=re.S)) for n in NEW_SYMBOLS)
    with open(os.path.join(CSRC, "build.sh")) as f:
        build = f.read()
    assert "tsu_hip_potts_muca.h" in build and "potts_muca_dev.h" in build and os.path.exists(os.path.join(CSRC, "potts_muca.hip"))
    with open(os.path.join(ROOT, "include", "tsu_hip_potts_muca.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tsu_potts_muca_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_hip.POTTS_MUCA_SIGNATURES)
    lib = _hip.load_library()
    for name in NEW_SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_hip.POTTS_MUCA_SIGNATURES[name][1]), name
        assert getattr(lib, name).argtypes == _hip.POTTS_MUCA_SIGNATURES[name][1]
        assert getattr(lib, name).restype is _hip.POTTS_MUCA_SIGNATURES[name][0]
    routes = [int(re.search(r"#define\s+TSU_POTTS_MUCA_ROUTE_" + n + r"\s+(\d+)\b", header).group(1)) for n in ("LDS", "GLOBAL", "ATOMICS")]
    assert routes == [0, 1, 2] and len(_hip.POTTS_MUCA_ROUTES) == 3
    assert int(re.search(r"#define\s+TSU_POTTS_MUCA_MAX_SITES\s+(\d+)\b", header).group(1)) == _hip.POTTS_MUCA_MAX_SITES == 65536
    assert int(re.search(r"#define\s+TSU_POTTS_MUCA_MAX_WALKERS\s+(\d+)\b", header).group(1)) == _hip.POTTS_MUCA_MAX_WALKERS == 2 ** 20
    # the new stream tag: 13, defined with the rule (tsu_common.h's enum stays 0 .. 12, as earlier tests pin it, and names no 13)
    with open(os.path.join(CSRC, "potts_muca_dev.h")) as f:
        assert re.search(r"TSU_TAG_POTTS_MUCA\s*=\s*13\b", f.read()) and mt.TAG_POTTS_MUCA == 13
    with open(os.path.join(CSRC, "tsu_common.h")) as f:
        assert sorted(int(v) for v in re.findall(r"TSU_TAG_[A-Z_]+\s*=\s*(\d+)", f.read())) == list(range(13))
    # a family of its own, disjoint from every other one (POTTS_SIGNATURES and POTTS3D_SIGNATURES stay as their headers pin them)
    families = {k: v for k, v in vars(_hip).items() if k.endswith("SIGNATURES") and isinstance(v, dict)}
    assert "POTTS_MUCA_SIGNATURES" in families
    for k, v in families.items():
        if k != "POTTS_MUCA_SIGNATURES":
            assert not set(v) & set(NEW_SYMBOLS), k
    import tsu
    from tsu import models
    for n in ("PottsMulticanonical", "potts_multicanonical_scan"):
        assert getattr(tsu, n) is getattr(models, n) and n in tsu.__all__ and n in models.__all__
    for n in ("weights", "spins", "fill", "run", "iterate", "histogram", "moments", "clear_record", "energies", "tunnels",
              "set_tunnel_bounds", "density_of_states", "reweight", "route", "launch_count", "close"):
        assert hasattr(tsu.PottsMulticanonical, n), n


def test_the_kernel_file_keeps_to_the_rule_and_to_plain_hip():
    src = open(os.path.join(CSRC, "potts_muca.hip")).read()
    assert '#include "potts_muca_dev.h"' in src and "muca_thresholds(" in src and "TSU_TAG_POTTS_MUCA" in src
    assert "k11_muca" in src and "k11_measure" in src
    code = re.sub(r"//[^\n]*", "", src)
    assert "asm" not in code and "hipLaunchCooperativeKernel" not in code and "exp(" not in code
    rule = open(os.path.join(CSRC, "potts_muca_dev.h")).read()
    assert "hip_runtime" not in rule and "__global__" not in rule and "muca_threshold(" in rule

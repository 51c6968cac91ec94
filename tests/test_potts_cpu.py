"""K10, the q-state Potts lattice, on the host (no GPU needed): the NumPy twin (tests/helpers/potts_twin.py) against exact
enumeration, the refusals ahead of the device, the new header and ctypes prototypes, and the decision rule of csrc/potts_dev.h
compiled for the host (with fused multiply-add available) against the twin."""
import importlib.util
import os
import re
import shutil
import subprocess

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


pt = _load("potts_twin")

NEW_SYMBOLS = ("tsu_potts2d_check_model", "tsu_potts2d_cluster_threshold", "tsu_potts2d_create", "tsu_potts2d_destroy",
               "tsu_potts2d_set_model", "tsu_potts2d_set_spins", "tsu_potts2d_get_spins", "tsu_potts2d_fill", "tsu_potts2d_sweep",
               "tsu_potts2d_cluster_sweep", "tsu_potts2d_route", "tsu_potts2d_measure", "tsu_potts2d_run", "tsu_potts2d_record",
               "tsu_potts2d_launch_count")

HEAT_BATH_CASES, CLUSTER_CASES = pt.ENUMERATION_HEAT_BATH, pt.ENUMERATION_CLUSTER


def test_plain_python_chain_equals_the_vectorised_twin():
    rng = np.random.default_rng(1)
    for shape, q, per, J, h, T in [((2, 3), 3, False, 1.0, (0.3, 0, -0.2), 1.5), ((4, 6), 5, True, -1.0, None, 0.8),
                                   ((2, 2), 8, True, 0.37, None, 2.0), ((1, 7), 2, False, 1.0, (0, 0.25), 1.0),
                                   ((7, 1), 3, False, 1.0, None, 1.0), ((2, 18), 3, True, 1.0, (0.1, 0.0, 0.2), 0.2)]:
        s = rng.integers(0, q, size=shape).astype(np.int8)
        a = pt.sweep(s, q, per, J, h, T, 6, 2 ** 63 + 12345, sweep0=2 ** 32 - 4, replica=3)
        b, _ = pt.chain(s, q, per, J, h, T, 6, 2 ** 63 + 12345, sweep0=2 ** 32 - 4, replica=3)
        assert (a == b).all(), shape
        assert a.min() >= 0 and a.max() < q
        if J > 0:
            a = pt.cluster_sweep(s, q, per, J, T, 6, 77, step0=5, replica=3)
            b, _ = pt.cluster_chain(s, q, per, J, T, 6, 77, step0=5, replica=3)
            assert (a == b).all(), ("cluster", shape)


@pytest.mark.parametrize("case", HEAT_BATH_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-q{c[1]}")
def test_twin_heat_bath_against_enumeration(case):
    """100 sweeps discarded, then 20 000 states, one every 4 sweeps; cells with expected count >= 5 one each, the rest pooled.
    The twin gives (the device equals it bit for bit, so these are the GPU test's numbers too):
      open 2x3 q=3 J=1  T=1.5 h=(0.3, 0, -0.2): chi2 = 689.8 on 665 dof, p = 0.245, pooled 1.2 %
      open 2x2 q=5 J=1  T=1.2 h=0:              chi2 = 597.3 on 624 dof, p = 0.772, pooled 0 %
      open 3x3 q=2 J=-1 T=1.0 h=(0, 0.25):      chi2 = 315.1 on 330 dof, p = 0.713, pooled 1.6 %
      open 1x3 q=8 J=1  T=2.0 h=0:              chi2 = 538.4 on 511 dof, p = 0.194, pooled 0 %"""
    shape, q, J, T, h, seed = case
    s, _ = pt.chain(np.zeros(shape, np.int8), q, False, J, h, T, 100, seed)
    s, codes = pt.chain(s, q, False, J, h, T, 80000, seed, sweep0=100, record_every=4)
    chi2, dof, p, pooled = pt.boltzmann_chi2(codes, shape, q, False, J, h, T)
    print(f"\n{shape} q={q}: chi2 = {chi2:.1f} on {dof} dof, p = {p:.3f}, pooled {100 * pooled:.1f} %")
    assert len(codes) == 20000 and p >= 0.01 and pooled <= 0.05


@pytest.mark.parametrize("case", CLUSTER_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-q{c[1]}")
def test_twin_cluster_steps_against_enumeration(case):
    """The same check for Swendsen-Wang steps at zero field.  The twin gives:
      open 2x3 q=3 J=1 T=1.5: chi2 = 699.1 on 675 dof, p = 0.253, pooled 1.1 %
      open 2x2 q=5 J=1 T=1.2: chi2 = 646.7 on 624 dof, p = 0.257, pooled 0 %"""
    shape, q, J, T, seed = case
    s, _ = pt.cluster_chain(np.zeros(shape, np.int8), q, False, J, T, 100, seed)
    s, codes = pt.cluster_chain(s, q, False, J, T, 80000, seed, step0=100, record_every=4)
    chi2, dof, p, pooled = pt.boltzmann_chi2(codes, shape, q, False, J, None, T)
    print(f"\n{shape} q={q}: chi2 = {chi2:.1f} on {dof} dof, p = {p:.3f}, pooled {100 * pooled:.1f} %")
    assert len(codes) == 20000 and p >= 0.01 and pooled <= 0.05


def test_measure_counts_a_double_bond_twice():
    s = np.array([[0, 1, 1, 0], [0, 1, 2, 0]], np.int8)
    n_eq, N = pt.measure(s, 3, True)
    # rows of length 4 (wrapping): row 0 has 1-1 and 0-0 across the wrap, row 1 has 0-0 across the wrap; the two rows are a periodic
    # axis of length 2: every column's bond counts twice (columns 0, 1 and 3 agree)
    assert n_eq == 2 + 1 + 2 * 3 and N.tolist() == [4, 3, 1]
    assert pt.measure(s, 3, False)[0] == 1 + 0 + 3
    assert pt.energy(s, 3, False, 2.0, (1.0, 0.0, -1.0)) == -2.0 * 4 - (4 - 1)
    assert pt.order_parameter(np.array([4, 3, 1]), 3) == pytest.approx((3 * 4 / 8 - 1) / 2)


def test_refusals_come_before_the_device(monkeypatch):
    import tsu
    from tsu import _hip
    from tsu.models import potts

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_hip.Context, "default", classmethod(no_device))
    monkeypatch.setattr(_hip, "PottsLattice", no_device)
    bad = [dict(q=1), dict(q=9), dict(q=2.5), dict(q=3, coupling=float("nan")), dict(q=3, coupling=float("inf")),
           dict(q=3, field=(0.0, float("nan"), 0.0)), dict(q=3, field=(0.0, 1.0)), dict(q=3, temperature=float("inf")),
           dict(q=3, temperature=float("nan")), dict(q=3, temperature=0.0), dict(q=3, temperature=-1.0),
           dict(q=3, coupling=150.5, temperature=1.0), dict(q=3, coupling=-1.0, field=(0.0, 598.0, 0.0), temperature=1.0),
           dict(q=2, size=(3, 4)), dict(q=2, size=(4, 5))]
    for kw in bad:
        args = dict(size=4, q=3)
        args.update(kw)
        with pytest.raises(tsu.ConfigurationError):
            tsu.PottsModel2D(**args)
    with pytest.raises(AssertionError, match="device was touched"):  # the largest model the bound lets through reaches the handle
        tsu.PottsModel2D(4, 3, coupling=150.0, temperature=1.0)
    with pytest.raises(AssertionError, match="device was touched"):
        tsu.PottsModel2D((3, 5), 3, periodic=False)
    for kw in (dict(temperatures=[1.0, -1.0]), dict(temperatures=[1.0], coupling=float("nan")), dict(temperatures=[0.001], coupling=1.0)):
        with pytest.raises(tsu.ConfigurationError):
            potts.potts_temperature_scan(4, 3, **kw)
    with pytest.raises(ValueError, match="algorithm"):
        potts.potts_temperature_scan(4, 3, [1.0], algorithm="wolff")
    # the library's own host-side check agrees, and so does the twin
    lib = _hip.load_library()
    assert lib.tsu_potts2d_check_model(3, 150.0, None, 1.0, None) == _hip.TSU_OK
    for q, J, h, T in ((1, 1.0, None, 1.0), (9, 1.0, None, 1.0), (3, float("nan"), None, 1.0), (3, 1.0, None, 0.0), (3, 1.0, None, float("inf")),
                       (3, 150.5, None, 1.0), (3, 1.0, (0.0, float("inf"), 0.0), 1.0), (3, 100.0, (0.0, 201.0, 0.0), 1.0)):
        hh = None if h is None else np.array(h, np.float64)
        assert lib.tsu_potts2d_check_model(q, J, None if hh is None else _hip._ptr(hh, _hip._f64p), T, None) == _hip.TSU_E_INVALID
        with pytest.raises(ValueError):
            pt.check_model(q, J, h, T)


def test_tables_and_threshold_of_the_library_equal_the_twin():
    from tsu import _hip
    rng = np.random.default_rng(3)
    for _ in range(200):
        q = int(rng.integers(2, 9))
        J = float(rng.normal()) * 2
        h = rng.normal(size=q)
        T = float(rng.uniform(0.2, 5.0))
        E, F = _hip.potts_tables(q, J, h, T)
        e, f = pt.tables(q, J, h, T)
        assert E.tobytes() == e.tobytes() and F.tobytes() == f.tobytes()
        assert _hip.potts_cluster_threshold(abs(J) + 0.01, T) == pt.threshold(abs(J) + 0.01, T)
    assert _hip.potts_cluster_threshold(1e6, 1.0) == 2 ** 32  # every satisfied bond active: the compare is 64-bit


def test_header_symbols_and_prototypes():
    from tsu import _hip
    with open(os.path.join(ROOT, "include", "tsu_hip.h")) as f:
        top = f.read()
    assert re.search(r'^#include "tsu_hip_potts.h"', top, flags=re.M)
    assert not any(re.search(r"\b" + n + r"\s*\(", re.sub(r"/\*.*?\*/", "", top, flags=re.S)) for n in NEW_SYMBOLS)
    with open(os.path.join(CSRC, "build.sh")) as f:
        build = f.read()
    assert "tsu_hip_potts.h" in build and "potts_dev.h" in build and "potts_host.h" in build
    with open(os.path.join(ROOT, "include", "tsu_hip_potts.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tsu_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_hip.POTTS_SIGNATURES)
    lib = _hip.load_library()
    for name in NEW_SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_hip.POTTS_SIGNATURES[name][1]), name
        assert getattr(lib, name).argtypes == _hip.POTTS_SIGNATURES[name][1]
        assert getattr(lib, name).restype is _hip.POTTS_SIGNATURES[name][0]
    assert re.search(r"#define\s+TSU_POTTS_RECORD_WORDS\s+9\b", header) and _hip.POTTS_RECORD_WORDS == 9
    assert re.search(r"#define\s+TSU_POTTS_MAX_Q\s+8\b", header) and _hip.POTTS_MAX_Q == 8
    families = {k: v for k, v in vars(_hip).items() if k.endswith("SIGNATURES") and isinstance(v, dict)}
    assert "POTTS_SIGNATURES" in families
    for k, v in families.items():
        if k != "POTTS_SIGNATURES":
            assert not set(v) & set(NEW_SYMBOLS), k
    import tsu
    from tsu import models
    for n in ("PottsModel2D", "potts_temperature_scan"):
        assert getattr(tsu, n) is getattr(models, n) and n in tsu.__all__ and n in models.__all__


def _compilers():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [c for c in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.exists(c)]
    return [c for c in (shutil.which("c++"), shutil.which("g++")) if c][:1] + found[:1]


def _build_rule_check(tmp_path):
    """The host compiler first (its default contracts a product and a sum across statements where the target has the
    instruction), each with -march=native when it takes it."""
    src = os.path.join(ROOT, "tests", "host", "potts_rule_check.cpp")
    exe = str(tmp_path / "potts_rule_check")
    errors = []
    for cxx in _compilers():
        for arch in (["-march=native"], []):
            r = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", *arch, "-I", CSRC, src, "-o", exe], capture_output=True, text=True)
            if r.returncode == 0:
                return exe
            errors.append(f"{cxx} {arch}: {r.stderr[-1500:]}")
    pytest.fail("no C++17 compiler built potts_rule_check.cpp:\n" + "\n".join(errors))


def test_rule_header_needs_no_hip_on_the_host():
    text = open(os.path.join(CSRC, "potts_dev.h")).read()
    assert "__dmul_rn" in text and "__dadd_rn" in text
    plain = re.sub(r"#if defined\(__HIPCC__\).*?#else", "", text, count=1, flags=re.S)
    assert sorted(re.findall(r"#\s*include\s*[<\"]([^>\"]+)", plain)) == ["math.h", "stdint.h"]
    kernels = open(os.path.join(CSRC, "potts_kern_dev.h")).read()  # the kernels of both handles; potts2d.hip instantiates them
    assert '#include "potts_dev.h"' in kernels and "potts_cum(" in kernels and "potts_pick(" in kernels
    assert '#include "potts_host.h"' in open(os.path.join(CSRC, "potts2d.hip")).read()
    assert '#include "potts_kern_dev.h"' in open(os.path.join(CSRC, "potts_host.h")).read()


def test_rule_on_the_host_equals_the_twin_without_a_fused_multiply_add(tmp_path):
    """Steps 2 - 4 through csrc/potts_dev.h itself on 10^5 inputs, four models of 25 000 each: random neighbour colours (missing
    ones included) and, for half of the inputs, a u on or next to a boundary Z_c 2^32 / Z_{q-1} (so that hi16 ties and the last
    bit of a product or a sum decide), the others uniform."""
    exe = _build_rule_check(tmp_path)
    rng = np.random.default_rng(7)
    total = 0
    for q, J, T, h in ((3, 1.0, 1.5, (0.3, 0.0, -0.2)), (8, 0.37, 0.9, tuple(rng.normal(size=8))), (2, -1.0, 0.2, (0.0, 0.25)),
                       (5, 1.0, 5.0, (0.0,) * 5)):
        n = 25000
        nb = rng.integers(-1, q, size=(4, n)).astype(np.int8)
        E, F = pt.tables(q, J, h, T)
        counts = [sum((x == c).astype(np.int64) for x in nb) for c in range(q)]
        Z = pt.cumulative(E, F, counts)
        u = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64)
        edge = rng.integers(0, q - 1, size=n) if q > 2 else np.zeros(n, np.int64)
        zc = np.choose(edge, Z[:q - 1]) if q > 2 else Z[0]
        near = np.floor(zc / Z[q - 1] * 4294967296.0).astype(np.int64) + rng.integers(-2, 3, size=n)
        tie = rng.random(n) < 0.5
        u = np.where(tie, np.clip(near, 0, 2 ** 32 - 1).astype(np.uint64), u).astype(np.uint32)
        want = pt.pick(Z, u)
        rec = np.zeros(n, dtype=[("nb", np.int8, 4), ("u", "<u4")])
        rec["nb"] = nb.T
        rec["u"] = u
        r = subprocess.run([exe, str(q), repr(J), repr(T)] + [repr(float(v)) for v in h], input=rec.tobytes(), capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.decode().splitlines()
        tab = np.array([float.fromhex(v) for v in lines[0].split()])
        assert tab[:5].tobytes() == E.tobytes() and tab[5:5 + q].tobytes() == F.tobytes()
        got = np.array(lines[1:], dtype=np.int64)
        assert got.shape == (n,) and (got == want).all(), (q, int(np.count_nonzero(got != want)))
        # the near-tie inputs did their work: both sides of a boundary occur among them
        assert len(set(want[tie].tolist())) >= 2
        total += n
    assert total == 100000

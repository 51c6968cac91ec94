"""K10 on the cubic lattice, on the host (no GPU needed): the NumPy twin (tests/helpers/potts3d_twin.py) against its plain-Python
chains, against the 2-D twin on one layer and against exact enumeration; the refusals ahead of the device; the new header and ctypes
prototypes; and the six-neighbour decision rule of csrc/potts_dev.h compiled for the host (with fused multiply-add available)
against the twin."""
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


p3 = _load("potts3d_twin")
p2 = _load("potts_twin")

NEW_SYMBOLS = ("tsu_potts3d_check_model", "tsu_potts3d_create", "tsu_potts3d_destroy", "tsu_potts3d_set_model", "tsu_potts3d_set_spins",
               "tsu_potts3d_get_spins", "tsu_potts3d_fill", "tsu_potts3d_sweep", "tsu_potts3d_cluster_sweep", "tsu_potts3d_route",
               "tsu_potts3d_measure", "tsu_potts3d_run", "tsu_potts3d_record", "tsu_potts3d_launch_count")


def _id(case):
    shape, q, per = case[0], case[1], case[2]
    return "x".join(map(str, shape)) + f"-q{q}-" + "".join("p" if x else "o" for x in per) + f"-J{case[3]:g}"


def test_plain_python_chain_equals_the_vectorised_twin():
    rng = np.random.default_rng(1)
    for shape, q, per, J, h, T in [((2, 2, 2), 3, False, 1.0, (0.3, 0, -0.2), 1.5), ((2, 2, 2), 2, True, -1.0, (0.0, 0.25), 0.8),
                                   ((4, 2, 6), 5, (True, True, True), -1.0, None, 0.8), ((2, 1, 3), 8, False, 0.37, None, 2.0),
                                   ((7, 1, 1), 2, False, 1.0, (0, 0.25), 1.0), ((3, 5, 7), 3, False, 1.0, None, 1.0),
                                   ((2, 2, 18), 3, True, 1.0, (0.1, 0.0, 0.2), 0.2), ((4, 5, 6), 3, (True, False, True), 1.0, None, 1.2),
                                   ((1, 6, 10), 5, (False, True, True), 1.0, None, 0.9)]:
        s = rng.integers(0, q, size=shape).astype(np.int8)
        a = p3.sweep(s, q, per, J, h, T, 6, 2 ** 63 + 12345, sweep0=2 ** 32 - 4, replica=3)
        b, _ = p3.chain(s, q, per, J, h, T, 6, 2 ** 63 + 12345, sweep0=2 ** 32 - 4, replica=3)
        assert (a == b).all(), shape
        assert a.min() >= 0 and a.max() < q
        if J > 0:
            a = p3.cluster_sweep(s, q, per, J, T, 6, 77, step0=5, replica=3)
            b, _ = p3.cluster_chain(s, q, per, J, T, 6, 77, step0=5, replica=3)
            assert (a == b).all(), ("cluster", shape)


def test_one_layer_equals_the_2d_twin():
    """(1, R, C) with periodic (False, p, p) is the 2-D model on (R, C): heat bath (with a field and J < 0), cluster steps, measure."""
    rng = np.random.default_rng(2)
    for (R, C), q, per, J, h, T in [((6, 10), 3, True, 1.0, (0.3, 0.0, -0.2), 1.1), ((5, 7), 8, False, -1.0, None, 0.7),
                                    ((2, 18), 2, True, 0.37, (0.0, 0.25), 2.0), ((4, 16), 5, True, 1.0, None, 0.9),
                                    ((33, 65), 3, False, 1.0, None, 1.0)]:
        s = rng.integers(0, q, size=(R, C)).astype(np.int8)
        per3 = (False, per, per)
        a = p3.sweep(s[None], q, per3, J, h, T, 4, 2 ** 64 - 59, sweep0=2 ** 32 - 2, replica=3)
        assert (a[0] == p2.sweep(s, q, per, J, h, T, 4, 2 ** 64 - 59, sweep0=2 ** 32 - 2, replica=3)).all(), (R, C)
        if J > 0:
            b = p3.cluster_sweep(s[None], q, per3, J, T, 4, 12345, step0=7, replica=3)
            assert (b[0] == p2.cluster_sweep(s, q, per, J, T, 4, 12345, step0=7, replica=3)).all(), ("cluster", R, C)
        n3, N3 = p3.measure(a, q, per3)
        n2, N2 = p2.measure(a[0], q, per)
        assert n3 == n2 and N3.tolist() == N2.tolist()
        assert p3.energy(a, q, per3, J, h) == p2.energy(a[0], q, per, J, h)
    # the first five table entries are the 2-D ones
    E3, F3 = p3.tables(3, 0.37, (0.1, 0.0, -0.1), 1.3)
    E2, F2 = p2.tables(3, 0.37, (0.1, 0.0, -0.1), 1.3)
    assert E3[:5].tobytes() == E2.tobytes() and F3.tobytes() == F2.tobytes()


def test_double_bonds_count_twice_on_each_axis():
    s = np.zeros((2, 2, 2), np.int8)
    for axis in range(3):
        per = tuple(a == axis for a in range(3))
        # 12 open bonds of the cube; the periodic axis of length 2 adds its 4 bonds a second time
        assert p3.measure(s, 2, per)[0] == 12 + 4, axis
        # one odd site: its bond along the periodic axis is lost twice, its two others once
        t = s.copy()
        t[0, 0, 0] = 1
        assert p3.measure(t, 2, per)[0] == 16 - 4 and p3.measure(t, 2, per)[1].tolist() == [7, 1]
        # the heat bath sees the double neighbour twice: site (0, 0, 0) has 4 neighbours, two of them the same site
        nb = p3.neighbours(t, per)
        assert sum(int(x[0, 0, 0] >= 0) for x in nb) == 4
        lists = p3._site_lists((2, 2, 2), per)
        assert len(lists[0]) == 4 and len(set(lists[0])) == 3
    assert p3.measure(s, 2, False)[0] == 12 and p3.measure(s, 2, True)[0] == 24
    s = np.array([[[0, 1]], [[0, 1]]], np.int8)  # (2, 1, 2): z periodic of length 2, two columns of equal colours
    assert p3.measure(s, 2, (True, False, False))[0] == 4 and p3.measure(s, 2, False)[0] == 2
    assert p3.energy(s, 2, (True, False, False), 2.0, (1.0, -1.0)) == -2.0 * 4 - 0.0
    # the cluster bonds too: both copies of the double bond are drawn (words of the sites at z = 0 and at z = 1), so at a threshold
    # where about half the words pass, the two sites of a column join more often than one bond would let them
    thr_T = 1.0 / np.log(2.0)  # p = 1 - exp(-J / T) = 1/2
    joined = sum(int(len(np.unique(p3.labels(s, (True, False, False), 1.0, thr_T, 5, t))) < 4) for t in range(400))
    single = sum(int(len(np.unique(p3.labels(s, False, 1.0, thr_T, 5, t))) < 4) for t in range(400))
    assert joined > single  # 1 - (1/4)^2 = 94 % of the steps against 1 - (1/2)^2 = 75 %


def test_refusals_come_before_the_device(monkeypatch):
    import tsu
    from tsu import _hip
    from tsu.models import potts

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_hip.Context, "default", classmethod(no_device))
    monkeypatch.setattr(_hip, "PottsLattice3D", no_device)
    bad = [dict(q=1), dict(q=9), dict(q=2.5), dict(q=3, coupling=float("nan")), dict(q=3, coupling=float("inf")),
           dict(q=3, field=(0.0, float("nan"), 0.0)), dict(q=3, field=(0.0, 1.0)), dict(q=3, temperature=float("inf")),
           dict(q=3, temperature=float("nan")), dict(q=3, temperature=0.0), dict(q=3, temperature=-1.0),
           dict(q=3, coupling=100.5, temperature=1.0), dict(q=3, coupling=-1.0, field=(0.0, 596.0, 0.0), temperature=1.0),
           dict(q=2, size=(3, 4, 4)), dict(q=2, size=(4, 5, 4)), dict(q=2, size=(4, 4, 5)), dict(q=2, size=(4, 4)),
           dict(q=2, size=(0, 4, 4)), dict(q=2, size=(1, 4, 4)), dict(q=2, size=(3, 4, 4), periodic=(True, False, False)),
           dict(q=2, periodic=(True, True)), dict(q=2, size=(2048, 1024, 1024), periodic=False), dict(q=3, initial=3),
           dict(q=3, initial="up"), dict(q=3, initial=-1)]
    for kw in bad:
        args = dict(size=4, q=3)
        args.update(kw)
        with pytest.raises(tsu.ConfigurationError):
            tsu.PottsModel3D(**args)
    # the largest model the six-neighbour bound lets through reaches the handle; so do odd open axes and one layer
    for kw in (dict(coupling=100.0, temperature=1.0), dict(size=(3, 5, 7), periodic=False), dict(size=(1, 4, 6), periodic=(False, True, True)),
               dict(size=(3, 4, 5), periodic=(False, True, False)), dict(initial=2)):
        args = dict(size=4, q=3)
        args.update(kw)
        with pytest.raises(AssertionError, match="device was touched"):
            tsu.PottsModel3D(**args)
    # the 2-D model keeps its four-neighbour bound
    monkeypatch.setattr(_hip, "PottsLattice", no_device)
    with pytest.raises(AssertionError, match="device was touched"):
        tsu.PottsModel2D(4, 3, coupling=150.0, temperature=1.0)
    for kw in (dict(temperatures=[1.0, -1.0]), dict(temperatures=[1.0], coupling=float("nan")), dict(temperatures=[0.001], coupling=1.0),
               dict(temperatures=[1.0], coupling=100.5)):
        with pytest.raises(tsu.ConfigurationError):
            potts.potts_temperature_scan_3d(4, 3, **kw)
    with pytest.raises(ValueError, match="algorithm"):
        potts.potts_temperature_scan_3d(4, 3, [1.0], algorithm="wolff")
    # the library's own host-side check agrees, and so does the twin
    lib = _hip.load_library()
    assert lib.tsu_potts3d_check_model(3, 100.0, None, 1.0, None) == _hip.TSU_OK
    for q, J, h, T in ((1, 1.0, None, 1.0), (9, 1.0, None, 1.0), (3, float("nan"), None, 1.0), (3, 1.0, None, 0.0), (3, 1.0, None, float("inf")),
                       (3, 100.5, None, 1.0), (3, 1.0, (0.0, float("inf"), 0.0), 1.0), (3, 66.0, (0.0, 205.0, 0.0), 1.0)):
        hh = None if h is None else np.array(h, np.float64)
        assert lib.tsu_potts3d_check_model(q, J, None if hh is None else _hip._ptr(hh, _hip._f64p), T, None) == _hip.TSU_E_INVALID
        with pytest.raises(ValueError):
            p3.check_model(q, J, h, T)
    # a common offset of h that carries exp(h_c / T) out of the float64 range is refused as in 2-D
    hh = np.array((700.0, 700.0, 700.0))
    assert lib.tsu_potts3d_check_model(3, 1.0, _hip._ptr(hh, _hip._f64p), 1.0, None) == _hip.TSU_E_INVALID


def test_tables_of_the_library_equal_the_twin():
    from tsu import _hip
    rng = np.random.default_rng(3)
    for _ in range(200):
        q = int(rng.integers(2, 9))
        J = float(rng.normal()) * 2
        h = rng.normal(size=q)
        T = float(rng.uniform(0.2, 5.0))
        E, F = _hip.potts3d_tables(q, J, h, T)
        e, f = p3.tables(q, J, h, T)
        assert E.shape == (7,) and E.tobytes() == e.tobytes() and F.tobytes() == f.tobytes()


def test_header_symbols_and_prototypes():
    from tsu import _hip
    with open(os.path.join(ROOT, "include", "tsu_hip.h")) as f:
        top = f.read()
    assert re.search(r'^#include "tsu_hip_potts3d.h"', top, flags=re.M)
    assert top.index('#include "tsu_hip_potts.h"') < top.index('#include "tsu_hip_potts3d.h"')
    assert not any(re.search(r"\b" + n + r"\s*\(", re.sub(r"/\*.*?\*/", "", top, flags=re.S)) for n in NEW_SYMBOLS)
    with open(os.path.join(CSRC, "build.sh")) as f:
        build = f.read()
    assert "tsu_hip_potts3d.h" in build and "potts_kern_dev.h" in build and os.path.exists(os.path.join(CSRC, "potts3d.hip"))
    with open(os.path.join(ROOT, "include", "tsu_hip_potts3d.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tsu_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_hip.POTTS3D_SIGNATURES)
    # symbol for symbol the 2-D header's, but for the threshold, which is shared
    assert sorted(n.replace("potts3d", "potts2d") for n in NEW_SYMBOLS) == sorted(set(_hip.POTTS_SIGNATURES) - {"tsu_potts2d_cluster_threshold"})
    lib = _hip.load_library()
    for name in NEW_SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_hip.POTTS3D_SIGNATURES[name][1]), name
        assert getattr(lib, name).argtypes == _hip.POTTS3D_SIGNATURES[name][1]
        assert getattr(lib, name).restype is _hip.POTTS3D_SIGNATURES[name][0]
        if name != "tsu_potts3d_create":
            assert _hip.POTTS3D_SIGNATURES[name] == _hip.POTTS_SIGNATURES[name.replace("potts3d", "potts2d")], name
    routes = [int(re.search(r"#define\s+TSU_POTTS3D_ROUTE_" + n + r"\s+(\d+)\b", header).group(1)) for n in ("SMALL", "SWEEP", "SW_SMALL", "SW_TILES")]
    assert routes == [0, 1, 2, 3] and len(_hip.POTTS3D_ROUTES) == 4
    families = {k: v for k, v in vars(_hip).items() if k.endswith("SIGNATURES") and isinstance(v, dict)}
    assert "POTTS3D_SIGNATURES" in families
    for k, v in families.items():
        if k != "POTTS3D_SIGNATURES":
            assert not set(v) & set(NEW_SYMBOLS), k
    import tsu
    from tsu import models
    for n in ("PottsModel3D", "potts_temperature_scan_3d"):
        assert getattr(tsu, n) is getattr(models, n) and n in tsu.__all__ and n in models.__all__
    for n in ("spins", "fill", "gibbs_update", "cluster_update", "equilibrate", "run", "colour_counts", "equal_bonds", "energy",
              "order_parameter", "route", "launch_count", "close"):
        assert hasattr(tsu.PottsModel3D, n) and hasattr(tsu.PottsModel2D, n), n


def _compilers():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [c for c in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.exists(c)]
    return [c for c in (shutil.which("c++"), shutil.which("g++")) if c][:1] + found[:1]


def _build_rule_check(tmp_path):
    """The host compiler first (its default contracts a product and a sum across statements where the target has the
    instruction), each with -march=native when it takes it."""
    src = os.path.join(ROOT, "tests", "host", "potts3d_rule_check.cpp")
    exe = str(tmp_path / "potts3d_rule_check")
    errors = []
    for cxx in _compilers():
        for arch in (["-march=native"], []):
            r = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", *arch, "-I", CSRC, src, "-o", exe], capture_output=True, text=True)
            if r.returncode == 0:
                return exe
            errors.append(f"{cxx} {arch}: {r.stderr[-1500:]}")
    pytest.fail("no C++17 compiler built potts3d_rule_check.cpp:\n" + "\n".join(errors))


def test_the_kernels_use_the_shared_rule():
    # one body for both dimensions: the kernels in potts_kern_dev.h, the host side in potts_host.h, instantiated by potts3d.hip
    kernels = open(os.path.join(CSRC, "potts_kern_dev.h")).read()
    assert '#include "potts_dev.h"' in kernels and "potts_cum(" in kernels and "potts_pick(" in kernels and "PottsTabN<2 * DIM>" in kernels
    host = open(os.path.join(CSRC, "potts_host.h")).read()
    assert '#include "potts_kern_dev.h"' in host and "potts_tables(" in host and "PottsTabN<2 * L::DIM>" in host
    unit = open(os.path.join(CSRC, "potts3d.hip")).read()
    assert '#include "potts_host.h"' in unit and "PottsHandle<3>" in unit and "potts_check_model<6>" in unit
    rule = open(os.path.join(CSRC, "potts_dev.h")).read()
    assert "struct PottsTabN" in rule and "double E[NB + 1]" in rule
    assert "using PottsTab6 = PottsTabN<6>" in rule and "using PottsTab = PottsTabN<4>" in rule  # E[7] and E[5]


def test_six_neighbour_rule_on_the_host_equals_the_twin_without_a_fused_multiply_add(tmp_path):
    """Steps 2 - 4 through csrc/potts_dev.h itself on 10^5 inputs, four models of 25 000 each: random neighbour colours (missing
    ones included, so n_c runs from 0 to 6) and, for half of the inputs, a u on or next to a boundary Z_c 2^32 / Z_{q-1} (so that
    hi16 ties and the last bit of a product or a sum decide), the others uniform."""
    exe = _build_rule_check(tmp_path)
    rng = np.random.default_rng(7)
    total = 0
    for q, J, T, h in ((3, 1.0, 1.5, (0.3, 0.0, -0.2)), (8, 0.37, 0.9, tuple(rng.normal(size=8))), (2, -1.0, 0.2, (0.0, 0.25)),
                       (5, 1.0, 5.0, (0.0,) * 5)):
        n = 25000
        nb = rng.integers(-1, q, size=(6, n)).astype(np.int8)
        nb[:, :q] = np.arange(q, dtype=np.int8)[None, :]  # six equal neighbours of every colour: n_c = 6 occurs
        E, F = p3.tables(q, J, h, T)
        counts = [sum((x == c).astype(np.int64) for x in nb) for c in range(q)]
        assert max(int(c.max()) for c in counts) == 6
        Z = p3.cumulative(E, F, counts)
        u = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64)
        edge = rng.integers(0, q - 1, size=n) if q > 2 else np.zeros(n, np.int64)
        zc = np.choose(edge, Z[:q - 1]) if q > 2 else Z[0]
        near = np.floor(zc / Z[q - 1] * 4294967296.0).astype(np.int64) + rng.integers(-2, 3, size=n)
        tie = rng.random(n) < 0.5
        u = np.where(tie, np.clip(near, 0, 2 ** 32 - 1).astype(np.uint64), u).astype(np.uint32)
        want = p3.pick(Z, u)
        rec = np.zeros(n, dtype=[("nb", np.int8, 6), ("pad", np.int8, 2), ("u", "<u4")])
        assert rec.dtype.itemsize == 12
        rec["nb"] = nb.T
        rec["u"] = u
        r = subprocess.run([exe, str(q), repr(J), repr(T)] + [repr(float(v)) for v in h], input=rec.tobytes(), capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.decode().splitlines()
        tab = np.array([float.fromhex(v) for v in lines[0].split()])
        assert tab[:7].tobytes() == E.tobytes() and tab[7:7 + q].tobytes() == F.tobytes()
        got = np.array(lines[1:], dtype=np.int64)
        assert got.shape == (n,) and (got == want).all(), (q, int(np.count_nonzero(got != want)))
        assert len(set(want[tie].tolist())) >= 2  # the near-tie inputs did their work: both sides of a boundary occur among them
        total += n
    assert total == 100000


def _heat_bath_chi2(case):
    shape, q, per, J, h, T, n_states, seed = case
    s, _ = p3.chain(np.zeros(shape, np.int8), q, per, J, h, T, 100, seed)
    s, codes = p3.chain(s, q, per, J, h, T, 4 * n_states, seed, sweep0=100, record_every=4)
    assert len(codes) == n_states
    return p3.boltzmann_chi2(codes, shape, q, per, J, h, T)


@pytest.mark.parametrize("case", p3.ENUMERATION_HEAT_BATH, ids=_id)
def test_twin_heat_bath_against_enumeration(case):
    """100 sweeps discarded, then 20 000 states, one every 4 sweeps; cells with expected count >= 5 one each, the rest pooled.
    The twin gives (the device equals it bit for bit, so these are the GPU test's numbers too):
      open 2x2x2 q=2 J=1   T=2.5 h=(0, 0.25):         chi2 = 271.9 on 255 dof, p = 0.223, pooled 0 %
      z-periodic 2x2x2 q=2 J=1 T=4.0 h=0:             chi2 = 250.4 on 255 dof, p = 0.569, pooled 0 %
      all-periodic 2x2x2 q=2 J=0.5 T=4.0 h=(0.1, -0.1): chi2 = 263.7 on 255 dof, p = 0.341, pooled 0 %
      open 2x2x2 q=2 J=-1  T=2.0 h=(0, 0.25):         chi2 = 263.7 on 254 dof, p = 0.325, pooled 0.03 %
      open 2x1x3 q=3 J=1   T=1.5 h=0:                 chi2 = 676.3 on 675 dof, p = 0.478, pooled 1.07 %"""
    chi2, dof, p, pooled = _heat_bath_chi2(case)
    print(f"\n{_id(case)}: chi2 = {chi2:.1f} on {dof} dof, p = {p:.3f}, pooled {100 * pooled:.2f} %")
    assert p >= 0.01 and pooled <= 0.05


def test_twin_heat_bath_against_enumeration_q3_cube():
    """Open 2x2x2, q = 3, J = 1, T = 2.5: 6561 cells, so 100 000 states (400 000 sweeps in plain Python); 20 000 would pool 59 % of
    the probability.  The twin gives:
      chi2 = 6224.7 on 6231 dof, p = 0.520, pooled 1.07 % (about 10 s here)"""
    case = p3.ENUMERATION_HEAT_BATH_LONG
    chi2, dof, p, pooled = _heat_bath_chi2(case)
    print(f"\n{_id(case)}: chi2 = {chi2:.1f} on {dof} dof, p = {p:.3f}, pooled {100 * pooled:.2f} %")
    assert p >= 0.01 and pooled <= 0.05


@pytest.mark.parametrize("case", p3.ENUMERATION_CLUSTER, ids=_id)
def test_twin_cluster_steps_against_enumeration(case):
    """The same check for Swendsen-Wang steps at zero field, 20 000 states 4 steps apart.  The twin gives:
      open 2x1x3 q=3 J=1 T=1.5: chi2 = 667.0 on 675 dof, p = 0.579, pooled 1.07 %
      open 2x2x2 q=2 J=1 T=2.5: chi2 = 233.9 on 255 dof, p = 0.824, pooled 0 %"""
    shape, q, per, J, T, n_states, seed = case
    s, _ = p3.cluster_chain(np.zeros(shape, np.int8), q, per, J, T, 100, seed)
    s, codes = p3.cluster_chain(s, q, per, J, T, 4 * n_states, seed, step0=100, record_every=4)
    chi2, dof, p, pooled = p3.boltzmann_chi2(codes, shape, q, per, J, None, T)
    print(f"\n{_id(case)}: chi2 = {chi2:.1f} on {dof} dof, p = {p:.3f}, pooled {100 * pooled:.2f} %")
    assert len(codes) == n_states and p >= 0.01 and pooled <= 0.05

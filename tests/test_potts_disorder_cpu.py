"""K12 on the host (no GPU needed): the rule of csrc/potts_disorder_dev.h built with the host compiler against the NumPy twin
(tests/helpers/potts_disorder_twin.py) and against the library's own tsu_potts_dis_site_thresholds, the twin against exact
enumeration, the refusals ahead of the device, the new header with its ctypes prototypes, and the assertion that no GPU case of
tests/test_potts_disorder_gpu.py holds a fragile decision."""
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


dt = _load("potts_disorder_twin")

NEW_SYMBOLS = ("tsu_potts_dis_site_thresholds", "tsu_potts_dis_create", "tsu_potts_dis_destroy", "tsu_potts_dis_set_disorder",
               "tsu_potts_dis_set_spins", "tsu_potts_dis_get_spins", "tsu_potts_dis_fill", "tsu_potts_dis_sweep",
               "tsu_potts_dis_cluster_sweep", "tsu_potts_dis_route", "tsu_potts_dis_measure", "tsu_potts_dis_run", "tsu_potts_dis_record",
               "tsu_potts_dis_launch_count")


def _compilers():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [c for c in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.exists(c)]
    return [c for c in (shutil.which("c++"), shutil.which("g++")) if c][:1] + found[:1]


def _build_rule_check(tmp_path):
    """The host compiler first, each with -march=native when it takes it (a contraction would then show), as test_potts_cpu.py
    builds its own."""
    src = os.path.join(ROOT, "tests", "host", "potts_disorder_rule_check.cpp")
    exe = str(tmp_path / "potts_disorder_rule_check")
    errors = []
    for cxx in _compilers():
        for arch in (["-march=native"], []):
            r = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", *arch, "-I", CSRC, src, "-o", exe], capture_output=True, text=True)
            if r.returncode == 0:
                return exe
            errors.append(f"{cxx} {arch}: {r.stderr[-1500:]}")
    pytest.fail("no C++17 compiler built potts_disorder_rule_check.cpp:\n" + "\n".join(errors))


def test_rule_header_needs_no_hip_on_the_host():
    text = open(os.path.join(CSRC, "potts_disorder_dev.h")).read()
    assert "__dadd_rn" not in text and "POTTS_ADD" in text and "__dsub_rn" in text and "__ddiv_rn" in text
    assert re.findall(r"#\s*include\s*[<\"]([^>\"]+)", text) == ["potts_dev.h"] and "__global__" not in text
    kernels = open(os.path.join(CSRC, "potts_disorder_kern_dev.h")).read()
    assert '#include "potts_disorder_dev.h"' in kernels and "pd_site_thresholds<" in kernels and "pd_pick(" in kernels
    for name in ("k12_sweep", "k12_small", "k12_measure", "k12_sw_small", "k12_sw_local", "k12_sw_merge", "k12_sw_resolve"):
        assert re.search(r"__global__[^;{]*\b" + name + r"\(", kernels), name
    code = re.sub(r"//[^\n]*", "", kernels + open(os.path.join(CSRC, "potts_disorder.hip")).read())
    assert "asm" not in code and "hipLaunchCooperativeKernel" not in code


@pytest.mark.parametrize("q,has_h", [(2, False), (2, True), (3, False), (3, True), (8, False), (8, True)])
def test_rule_on_the_host_equals_the_twin_and_the_library(tmp_path_factory, q, has_h):
    """Steps 1 - 5 through csrc/potts_disorder_dev.h itself on 20 000 random sites per model (missing neighbours included; half of
    the u on or next to a threshold), threshold for threshold and colour for colour; tsu_potts_dis_site_thresholds gives the same
    thresholds for the first 2000 sites' sums."""
    from tsu import _hip
    exe = _build_rule_check(tmp_path_factory.mktemp("rule"))
    rng = np.random.default_rng(40 + q + has_h)
    n, T = 20000, float(rng.uniform(0.3, 3.0))
    nb = rng.integers(-1, q, size=(n, 6)).astype(np.int8)
    J = (rng.normal(size=(n, 6)) * rng.choice([0.2, 1.0, 5.0], size=(n, 1))).astype(np.float32)
    hv = np.zeros((n, 8), np.float32)
    if has_h:
        hv[:, :q] = rng.normal(size=(n, q)).astype(np.float32)
    a = hv[:, :q].astype(np.float64).T.copy()
    for c in range(q):
        for k in range(6):
            a[c] = np.where(nb[:, k] == c, a[c] + J[:, k].astype(np.float64), a[c])
    thr, real = dt.thresholds(a, T)
    edge = rng.integers(0, q - 1, size=n)
    near = thr[edge, np.arange(n)].astype(np.int64) + rng.integers(-2, 3, size=n)
    u = np.where(rng.random(n) < 0.5, np.clip(near, 0, 2 ** 32 - 1), rng.integers(0, 2 ** 32, size=n)).astype(np.uint32)
    want = dt.pick(thr, u)
    rec = np.zeros(n, dtype=[("nb", np.int8, 6), ("pad", np.int8, 2), ("J", "<f4", 6), ("h", "<f4", 8), ("u", "<u4")])
    rec["nb"], rec["J"], rec["h"], rec["u"] = nb, J, hv, u
    assert rec.dtype.itemsize == 68
    r = subprocess.run([exe, str(q), repr(T), str(int(has_h))], input=rec.tobytes(), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.array([line.split() for line in r.stdout.decode().splitlines()], dtype=np.uint64)
    assert got.shape == (n, 1 + q)
    assert (got[:, 1:].T == thr).all() and (got[:, 0].astype(np.int8) == want).all()
    assert (thr[q - 1] == 2 ** 32).all() and (np.diff(thr.astype(np.int64), axis=0) >= 0).all() and len(set(want.tolist())) == q
    for i in range(2000):
        assert _hip.potts_site_thresholds(a[:, i], T).tolist() == thr[:, i].tolist() == dt.site_thresholds(a[:, i], T)


def test_site_thresholds_at_the_edges_of_the_rule():
    from tsu import _hip
    # equal sums: thr_c = (c + 1) 2^32 / q rounded; a sum far below the maximum underflows to weight 0 and never wins
    assert _hip.potts_site_thresholds([0.5, 0.5, 0.5, 0.5], 1.0).tolist() == [2 ** 30, 2 ** 31, 3 * 2 ** 30, 2 ** 32]
    assert _hip.potts_site_thresholds([-5000.0, 0.0], 1.0).tolist() == [0, 2 ** 32]
    assert _hip.potts_site_thresholds([0.0, -5000.0], 1.0).tolist() == [2 ** 32, 2 ** 32]
    assert _hip.potts_site_thresholds([1e300, 1e300], 1e-300).tolist() == [2 ** 31, 2 ** 32]  # nothing overflows
    for bad in (([0.0], 1.0), ([0.0] * 9, 1.0), ([0.0, float("nan")], 1.0), ([0.0, 1.0], 0.0), ([0.0, 1.0], float("inf")), ([0.0, 1.0], -1.0)):
        with pytest.raises(ValueError):
            _hip.potts_site_thresholds(*bad)


def test_plain_python_chains_equal_the_vectorised_twin():
    rng = np.random.default_rng(2)
    for shape, per, q in (((2, 3), False, 3), ((2, 2, 2), False, 2), ((2, 2), True, 4), ((2, 2, 4), True, 3)):
        s = rng.integers(0, q, size=shape).astype(np.int8)
        J, h = dt.random_disorder(shape, per, q, rng, "gaussian", True)
        a, fa = dt.sweep(s, q, per, J, h, 1.1, 7, 99, sweep0=2 ** 32 - 3, replica=2, with_fragile=True)
        b, _, fb = dt.chain(s, q, per, J, h, 1.1, 7, 99, sweep0=2 ** 32 - 3, replica=2)
        assert (a == b).all() and fa == fb == 0 and (a != s).any()
        J, _ = dt.random_disorder(shape, per, q, rng, "012", False)
        a, fa = dt.cluster_sweep(s, q, per, J, 1.3, 7, 99, step0=5, replica=2, with_fragile=True)
        b, _, fb = dt.cluster_chain(s, q, per, J, 1.3, 7, 99, step0=5, replica=2)
        assert (a == b).all() and fa == fb == 0


def test_energy_orders_and_measure():
    """The device's fixed order against one exact sum, on a lattice of more than one workgroup's worth of sites and more than one
    partial per lane of the final pass; a double bond holds two stored couplings and both count."""
    rng = np.random.default_rng(3)
    for shape, per, q in (((70, 66), False, 3), ((2, 2), True, 2), ((3, 5, 7), False, 8), ((2, 4, 16), True, 3), ((520, 520), True, 2)):
        s = rng.integers(0, q, size=shape).astype(np.int8)
        J, h = dt.random_disorder(shape, per, q, rng, "gaussian", True)
        e, p = dt.energy(s, q, per, J, h), dt.energy_plain(s, q, per, J, h)
        assert abs(e - p) <= 1e-12 * abs(p)
    s = np.zeros((2, 2), np.int8)
    J = (np.array([[1.0, 2.0], [4.0, 8.0]], np.float32), np.array([[16.0, 32.0], [64.0, 128.0]], np.float32))
    assert dt.energy(s, 2, True, J) == -255.0 and dt.measure(s, 2, True)[0] == 8
    s[0, 0] = 1
    assert dt.energy(s, 2, True, J) == -(4.0 + 8.0 + 32.0 + 128.0)


def _enum_id(case):
    return "x".join(map(str, case[0])) + f"-q{case[1]}-" + case[3]


@pytest.mark.parametrize("case", dt.ENUMERATION_HEAT_BATH, ids=_enum_id)
def test_twin_heat_bath_against_enumeration(case):
    """K10's protocol: 100 sweeps discarded, 20 000 states 4 sweeps apart, from colour 0, against exp(-E / T) / Z over all q^N states;
    p >= 0.01, at most 5 % pooled.  The twin gives (the device repeats the chains bit for bit, tests/test_potts_disorder_gpu.py):
      open 2x3 q=3, Gaussian couplings of both signs and a Gaussian site field:  chi2 = 493.6 on 533 dof, p = 0.888, pooled 2.49 %
      open 2x2x2 q=2, the same kind of disorder:                                 chi2 = 284.5 on 250 dof, p = 0.066, pooled 0.11 %
    No decision of either chain is fragile."""
    shape, q, per, kind, field, T, dseed, seed = case
    J, h = dt.enumeration_disorder(case)
    assert min(a.min() for a in J) < 0 < max(a.max() for a in J) and h is not None
    s, _, f0 = dt.chain(np.zeros(shape, np.int8), q, per, J, h, T, dt.N_DISCARD, seed)
    _, codes, f1 = dt.chain(s, q, per, J, h, T, dt.N_STATES * dt.EVERY, seed, sweep0=dt.N_DISCARD, record_every=dt.EVERY)
    chi2, dof, p, pooled = dt.boltzmann_chi2(codes, shape, q, per, J, h, T)
    print(f"\n{_enum_id(case)}: chi2 = {chi2:.1f} on {dof} dof, p = {p:.3f}, pooled {100 * pooled:.2f} %")
    assert f0 + f1 == 0 and len(codes) == dt.N_STATES and p >= 0.01 and pooled <= 0.05


@pytest.mark.parametrize("case", dt.ENUMERATION_CLUSTER, ids=_enum_id)
def test_twin_cluster_steps_against_enumeration(case):
    """The same for Swendsen-Wang chains on couplings from {0, 1, 2} (a diluted bond is never active):
      open 2x3 q=3:  chi2 = 543.7 on 585 dof, p = 0.888, pooled 1.42 %"""
    shape, q, per, kind, field, T, dseed, seed = case
    J, _ = dt.enumeration_disorder(case)
    assert {0.0, 1.0, 2.0} >= set(np.concatenate([a.ravel() for a in J]).tolist()) and any((a == 0).any() for a in J)
    s, _, f0 = dt.cluster_chain(np.zeros(shape, np.int8), q, per, J, T, dt.N_DISCARD, seed)
    _, codes, f1 = dt.cluster_chain(s, q, per, J, T, dt.N_STATES * dt.EVERY, seed, step0=dt.N_DISCARD, record_every=dt.EVERY)
    chi2, dof, p, pooled = dt.boltzmann_chi2(codes, shape, q, per, J, None, T)
    print(f"\n{_enum_id(case)}: chi2 = {chi2:.1f} on {dof} dof, p = {p:.3f}, pooled {100 * pooled:.2f} %")
    assert f0 + f1 == 0 and len(codes) == dt.N_STATES and p >= 0.01 and pooled <= 0.05


def test_no_gpu_case_holds_a_fragile_decision():
    """Only a decision whose u lies within one unit of its real-valued threshold can depend on whose exp or expm1 ran; every
    bit-for-bit case of the GPU file has none (about 3 (q - 1) 2^-32 each: any seed should do, and these do)."""
    decisions = 0
    for case in dt.heat_bath_cases():
        s, J, h = dt.case_inputs(case)
        out, f = dt.sweep(s, case["q"], case["periodic"], J, h, case["T"], dt.N_UPDATES, case["seed"], case["sweep0"], case["replica"], True)
        assert f == 0 and (out != s).any(), dt.case_id(case)
        decisions += dt.N_UPDATES * s.size * (case["q"] - 1)
    for case in dt.cluster_cases():
        s, J, _ = dt.case_inputs(case)
        out, f = dt.cluster_sweep(s, case["q"], case["periodic"], J, case["T"], dt.N_UPDATES, case["seed"], case["sweep0"], case["replica"], True)
        assert f == 0 and (out != s).any(), dt.case_id(case)
        # constant J = 1 against K10's cluster steps on the same colours
        ones = dt.constant_couplings(case["shape"], case["periodic"], 1.0)
        assert dt.cluster_sweep(s, case["q"], case["periodic"], ones, case["T"], dt.N_UPDATES, case["seed"], case["sweep0"], case["replica"], True)[1] == 0
    assert decisions > 40000


def test_refusals_come_before_the_device(monkeypatch):
    import tsu
    from tsu import _hip
    from tsu.models import potts

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_hip.Context, "default", classmethod(no_device))
    monkeypatch.setattr(_hip, "PottsDisorderLattice", no_device)
    monkeypatch.setattr(_hip, "PottsLattice", no_device)
    monkeypatch.setattr(_hip, "PottsLattice3D", no_device)
    ok2 = (np.zeros((4, 4)), np.zeros((4, 4)))
    ok3 = (np.zeros((4, 4, 4)),) * 3
    open_jr = np.ones((3, 5))
    open_jr[:, -1] = 0
    open_jd = np.ones((3, 5))
    open_jd[-1] = 0
    nan = np.zeros((4, 4))
    nan[1, 2] = float("nan")
    bad2 = [dict(couplings=ok2[:1]), dict(couplings=ok2 + ok2[:1]), dict(couplings=(np.zeros((4, 5)), np.zeros((4, 4)))),
            dict(couplings=(nan, ok2[1])), dict(couplings=(np.full((4, 4), 1e39), ok2[1])), dict(couplings=ok2, coupling=2.0),
            dict(site_field=np.zeros((4, 4, 2))), dict(site_field=np.zeros((4, 4))), dict(site_field=np.full((4, 4, 3), float("inf"))),
            dict(site_field=np.full((4, 4, 3), -1e39)), dict(site_field=np.zeros((4, 4, 3)), field=(0.0, 1.0, 0.0)),
            dict(couplings=ok2, temperature=0.0), dict(couplings=ok2, temperature=float("nan")), dict(couplings=ok2, q=9),
            dict(couplings=ok2, q=1), dict(size=(3, 5), periodic=False, couplings=(np.ones((3, 5)), open_jd)),
            dict(size=(3, 5), periodic=False, couplings=(open_jr, np.ones((3, 5)))), dict(size=(3, 4), couplings=(np.zeros((3, 4)),) * 2)]
    for kw in bad2:
        args = dict(size=4, q=3)
        args.update(kw)
        with pytest.raises(tsu.ConfigurationError):
            tsu.PottsModel2D(**args)
    bad3 = [dict(couplings=ok3[:2]), dict(couplings=ok3, coupling=0.5), dict(site_field=np.zeros((4, 4, 4))),
            dict(periodic=(False, True, True), couplings=(ok3[0], ok3[1], np.ones((4, 4, 4)))), dict(couplings=ok3, temperature=-1.0)]
    for kw in bad3:
        args = dict(size=4, q=3)
        args.update(kw)
        with pytest.raises(tsu.ConfigurationError):
            tsu.PottsModel3D(**args)
    # what is legal reaches the handle: huge couplings over a tiny T (no 600 bound), an open lattice with its last slices 0, a site
    # field alone, a per-colour field spread over the sites of a random-bond model
    for cls, kw in ((tsu.PottsModel2D, dict(couplings=(np.full((4, 4), 1e30), np.full((4, 4), -1e30)), temperature=1e-30)),
                    (tsu.PottsModel2D, dict(size=(3, 5), periodic=False, couplings=(open_jr, open_jd))),
                    (tsu.PottsModel2D, dict(site_field=np.ones((4, 4, 3)))),
                    (tsu.PottsModel2D, dict(couplings=ok2, field=(0.0, 1.0, 0.0))),
                    (tsu.PottsModel3D, dict(couplings=ok3, site_field=np.zeros((4, 4, 4, 3))))):
        args = dict(size=4, q=3)
        args.update(kw)
        with pytest.raises(AssertionError, match="device was touched"):
            cls(**args)
    for kw in (dict(temperatures=[1.0, -1.0], couplings=ok2), dict(temperatures=[1.0], couplings=ok2[:1])):
        with pytest.raises(tsu.ConfigurationError):
            potts.potts_temperature_scan(4, 3, **kw)
    with pytest.raises(AssertionError, match="device was touched"):
        potts.potts_temperature_scan(4, 3, [1.0], couplings=ok2)
    with pytest.raises(AssertionError, match="device was touched"):
        potts.potts_temperature_scan_3d(4, 3, [1.0], site_field=np.zeros((4, 4, 4, 3)))
    # without the new arguments the constructors do what they did: K10's bound still holds, and K10's handle is the one created
    with pytest.raises(tsu.ConfigurationError):
        tsu.PottsModel2D(4, 3, coupling=150.5, temperature=1.0)
    with pytest.raises(AssertionError, match="device was touched"):
        tsu.PottsModel2D(4, 3, coupling=150.0, temperature=1.0)
    # the arrays the device would get: rounded once to fp32, the field colour-major
    J, h = potts.potts_disorder_arrays((3, 5), 3, (False, False), (open_jr * 0.1, open_jd * 0.1), np.arange(45.0).reshape(3, 5, 3))
    assert all(a.dtype == np.float32 and a.flags.c_contiguous for a in J + (h,)) and J[0][0, 0] == np.float32(0.1)
    assert h.shape == (3, 3, 5) and h[2, 1, 4] == 3 * (1 * 5 + 4) + 2
    J, h = potts.potts_disorder_arrays((2, 4, 4), 3, (True, False, True), None, np.zeros((2, 4, 4, 3)), coupling=-0.5)
    assert (J[0] == -0.5).all() and (J[1][:, -1] == 0).all() and (J[1][:, :-1] == -0.5).all() and (J[2] == -0.5).all()


def test_header_symbols_and_prototypes():
    from tsu import _hip
    with open(os.path.join(ROOT, "include", "tsu_hip.h")) as f:
        top = f.read()
    assert re.search(r'^#include "tsu_hip_potts_disorder.h"', top, flags=re.M)
    assert top.index('#include "tsu_hip_potts_muca.h"') < top.index('#include "tsu_hip_potts_disorder.h"')
    assert not any(re.search(r"\b" + n + r"\s*\(", re.sub(r"/\*.*?\*/", "", top, flags=re.S)) for n in NEW_SYMBOLS)
    with open(os.path.join(CSRC, "build.sh")) as f:
        build = f.read()
    assert "tsu_hip_potts_disorder.h" in build and "potts_disorder_dev.h" in build and "potts_disorder_kern_dev.h" in build
    assert os.path.exists(os.path.join(CSRC, "potts_disorder.hip"))
    with open(os.path.join(ROOT, "include", "tsu_hip_potts_disorder.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tsu_potts_dis_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_hip.POTTS_DISORDER_SIGNATURES)
    lib = _hip.load_library()
    for name in NEW_SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_hip.POTTS_DISORDER_SIGNATURES[name][1]), name
        assert getattr(lib, name).argtypes == _hip.POTTS_DISORDER_SIGNATURES[name][1]
        assert getattr(lib, name).restype is _hip.POTTS_DISORDER_SIGNATURES[name][0]
    routes = [int(re.search(r"#define\s+TSU_POTTS_DIS_ROUTE_" + n + r"\s+(\d+)\b", header).group(1)) for n in ("SMALL", "SWEEP", "SW_SMALL", "SW_TILES")]
    assert routes == [0, 1, 2, 3] and _hip.POTTS_DIS_ROUTES == ("k12_small", "k12_sweep", "k12_sw_small", "k12_sw_tiles")
    assert int(re.search(r"#define\s+TSU_POTTS_DIS_RECORD_WORDS\s+(\d+)\b", header).group(1)) == _hip.POTTS_DIS_RECORD_WORDS == 10
    # no new stream tag: tsu_common.h's enum stays 0 .. 12
    with open(os.path.join(CSRC, "tsu_common.h")) as f:
        assert sorted(int(v) for v in re.findall(r"TSU_TAG_[A-Z_]+\s*=\s*(\d+)", f.read())) == list(range(13))
    assert "TSU_TAG_" not in re.sub(r"TSU_TAG_(ISING_HI|ISING_LO)\b", "", open(os.path.join(CSRC, "potts_disorder.hip")).read())
    # a family of its own, disjoint from every other one
    families = {k: v for k, v in vars(_hip).items() if k.endswith("SIGNATURES") and isinstance(v, dict)}
    assert "POTTS_DISORDER_SIGNATURES" in families
    for k, v in families.items():
        if k != "POTTS_DISORDER_SIGNATURES":
            assert not set(v) & set(NEW_SYMBOLS), k
    import inspect
    import tsu
    for cls in (tsu.PottsModel2D, tsu.PottsModel3D):
        params = inspect.signature(cls.__init__).parameters
        assert params["couplings"].kind is params["site_field"].kind is inspect.Parameter.KEYWORD_ONLY
        assert hasattr(cls, "set_disorder")
    from tsu.models import potts
    for fn in (potts.potts_temperature_scan, potts.potts_temperature_scan_3d):
        params = inspect.signature(fn).parameters
        assert params["couplings"].kind is params["site_field"].kind is inspect.Parameter.KEYWORD_ONLY

"""K14 on the host (no GPU needed): the twin's population (tests/helpers/potts_pop_twin.py) against the twins it composes; the device
draw by hand; the assertion that no bit-for-bit GPU case of tests/test_potts_pop_gpu.py holds a fragile decision; the free energy on a
synthetic record; the packing rule (csrc/potts_pop_plan.h) as a stand-alone host program, plain and under the sanitizers, against its
Python mirror; the new header with its ctypes prototypes and the build list; the Python refusals ahead of the device; and the
enumeration criterion of the GPU test on the statistical reference."""
import importlib.util
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "tsu-emulator_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "host", "potts_pop_plan_check.cpp")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


pp = _load("potts_pop_twin")
pdt, pop = pp.pdt, pp.pop

NEW_SYMBOLS = ("tsu_potts_pop_create", "tsu_potts_pop_destroy", "tsu_potts_pop_set_disorder", "tsu_potts_pop_set_schedule",
               "tsu_potts_pop_init", "tsu_potts_pop_advance", "tsu_potts_pop_run", "tsu_potts_pop_history", "tsu_potts_pop_energies",
               "tsu_potts_pop_get_spins", "tsu_potts_pop_set_spins", "tsu_potts_pop_get_padded", "tsu_potts_pop_route", "tsu_potts_pop_plan", "tsu_potts_pop_launch_count")


def test_twin_chain_is_the_shared_twins_step_by_step():
    """A resampled chain of the twin: every step passes population_twin.check_step on its own record, every plane is its parent's
    plane swept by potts_disorder_twin.sweep with the child's key, E / n_eq / N are potts_disorder_twin's, and steps kill and multiply."""
    c = pp.CHAIN_CASES[1]
    J, h = pdt.random_disorder(c["shape"], c["periodic"], c["q"], np.random.default_rng(c["dseed"]), "gaussian", c["field"])
    betas = [0.0, 0.6, 1.4, 2.4]
    tw = pp.Population(c["shape"], c["q"], c["periodic"], J, h, betas, c["seed"], 33)
    assert (tw.spins == pp.draw(c["shape"], c["q"], c["seed"], 33)).all()
    before = tw.spins.copy()
    died = 0
    for j in range(3):
        rec = tw.run(1, 2)
        parent = pop.check_step(rec["E"][0], rec["W"][0], betas[j + 1] - betas[j], j, c["seed"], rec["S"][0], rec["U"][0], rec["E_min"][0],
                                rec["parent"][0])
        n = np.bincount(parent, minlength=33)
        assert n.sum() == 33 and (parent[n > 0] == np.flatnonzero(n > 0)).all()
        died += int((n == 0).sum())
        for i in (0, 7, 32):
            want = pdt.sweep(before[parent[i]], c["q"], c["periodic"], J, h, 1.0 / betas[j + 1], 2, c["seed"] + i, 2 * j, 0)
            assert (tw.spins[i] == want).all()
            assert rec["E"][1, i] == pdt.energy(want, c["q"], c["periodic"], J, h)
            n_eq, N = pdt.measure(want, c["q"], c["periodic"])
            assert rec["n_eq"][1, i] == n_eq and (rec["N"][1, i] == N[:c["q"]]).all() and rec["N"][1, i].sum() == 12
        before = tw.spins.copy()
    assert died > 0 and tw.sweeps == 6 and tw.step == 3


def test_the_draw_by_hand():
    """Site (rho, c) of walker i: ((uint64) W q) >> 32 with W = word c & 3 of Philox(c >> 2, rho, 0, TAG_INIT = 2), key seed + i,
    computed one site at a time with Python integers; every colour occurs, and the key wraps at 2^64."""
    for shape, q, seed in (((5, 37), 3, 2 ** 64 - 2), ((3, 4, 18), 8, 12345), ((16, 16), 2, 0x9E3779B97F4A7C15)):
        got = pp.draw(shape, q, seed, 4)
        assert got.shape == (4,) + shape and got.dtype == np.int8 and sorted(np.unique(got)) == list(range(q))
        flat = got.reshape(4, -1, shape[-1])
        rng = np.random.default_rng(1)
        for _ in range(40):
            i, rho, c = int(rng.integers(4)), int(rng.integers(flat.shape[1])), int(rng.integers(shape[-1]))
            key = (seed + i) % 2 ** 64
            w = pop.philox(c >> 2, rho, 0, 2, key & 0xFFFFFFFF, key >> 32)
            assert flat[i, rho, c] == (int(w[c & 3]) * q) >> 32 == pp.draw_colour(int(w[c & 3]), q)
        assert (got[0] != got[1]).any()
    assert pp.draw_colour(2 ** 32 - 1, 8) == 7 and pp.draw_colour(0, 8) == 0 and pp.draw_colour(2 ** 31, 3) == 1


@pytest.mark.parametrize("c", pp.single_cases(), ids=pp.case_id)
def test_single_cases_hold_no_fragile_decision(c):
    tw = pp.single_twin(c)
    tw.run(3, pp.SWEEPS_PER_STEP, resample=False)
    assert tw.fragile == 0 and len(tw.walkers) >= 3


@pytest.mark.parametrize("c", pp.CHAIN_CASES, ids=lambda c: "x".join(map(str, c["shape"])) + f"-q{c['q']}-R{c['R']}-db{c['db']}")
def test_chain_cases_hold_no_fragile_decision_and_move_walkers(c):
    J, h = pdt.random_disorder(c["shape"], c["periodic"], c["q"], np.random.default_rng(c["dseed"]), "gaussian", c["field"])
    tw = pp.Population(c["shape"], c["q"], c["periodic"], J, h, pp.chain_betas(c), c["seed"], c["R"], initial_sweeps=1)
    rec = tw.run(pp.CHAIN_STEPS, pp.CHAIN_SWEEPS)
    assert tw.fragile == 0
    moved = (rec["parent"] != np.arange(c["R"])).any()
    assert moved == (c["db"] > 1e-6)  # a step of 1e-9 leaves every weight at 2^30 or one unit below: nobody dies


def test_free_energy_on_a_synthetic_record():
    from tsu.models import potts_population as mod
    from tsu.models.ising import population_free_energy
    betas = np.array([0.0, 0.5, 1.25])
    S = np.array([3 << 29, 5 << 28], np.uint64)
    E_min = np.array([-7.5, -9.0])
    mean_E = np.array([-1.0, -5.0, -8.0])
    fe = mod.potts_population_free_energy(betas, S, E_min, mean_E, 4, 12, 3)
    want = [12 * math.log(3.0)]
    want.append(want[0] + 0.5 * 7.5 + math.log((3 << 29) / (4.0 * (1 << 30))))
    want.append(want[1] + 0.75 * 9.0 + math.log((5 << 28) / (4.0 * (1 << 30))))
    assert fe["ln_Z"][0] == 12 * np.log(3.0) and np.allclose(fe["ln_Z"], want, rtol=0, atol=1e-12)
    assert np.isnan(fe["F"][0]) and np.allclose(fe["F"][1:], -np.array(want[1:]) / betas[1:]) and np.allclose(fe["entropy"], betas * mean_E + want)
    assert np.allclose(pp.free_energy(list(betas), S, E_min, mean_E, 4, 12, 3), want, rtol=0, atol=1e-12)
    # q = 2 is the Ising populations' estimator, which has not moved
    ising = population_free_energy(betas, S, E_min, mean_E, 4, 12)
    two = mod.potts_population_free_energy(betas, S, E_min, mean_E, 4, 12, 2)
    assert all(np.array_equal(ising[k], two[k], equal_nan=True) for k in ising) and ising["ln_Z"][0] == 12 * np.log(2.0)
    # differences only from beta[0] > 0
    d = mod.potts_population_free_energy(betas + 0.1, S, E_min, mean_E, 4, 12, 3)
    assert d["ln_Z"][0] == 0.0 and np.isnan(d["F"]).all() and np.isnan(d["entropy"]).all()


def _compilers():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [c for c in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.exists(c)]
    return found[:1] + [c for c in (shutil.which("c++"),) if c]


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    errors = []
    for cxx in _compilers():
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, *flags, SOURCE, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            break
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    else:
        pytest.fail("no C++17 compiler built potts_pop_plan_check.cpp:\n" + "\n".join(errors))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


def _fold(h, v):
    return ((h * 1099511628211) & pp.MASK64) ^ (v & pp.MASK64)


def _mirror_lines():
    lines = []
    for sites in range(1, 16401):
        h = 1469598103934665603
        for n_lanes in ((sites + 15) // 16, sites):
            for dim in (2, 3):
                for q in range(2, 9):
                    for field in (0, 1):
                        for R in (2, 3, 255, 65535):
                            for v in pp.plan(sites, n_lanes, dim, q, field, R):
                                h = _fold(h, v)
        lines.append(f"{sites} {h:016x}")
    for s in ((256, 16, 2, 3, 0), (256, 16, 2, 8, 1), (1024, 64, 2, 8, 1), (512, 64, 3, 8, 1), (4096, 256, 3, 3, 0), (192, 12, 2, 3, 1)):
        lines.append("plan " + " ".join(map(str, s)) + ": " + " ".join(map(str, pp.plan(*s, 70))))
    return lines + ["0 failed"]


def test_packing_rule_header_needs_no_hip():
    text = open(os.path.join(CSRC, "potts_pop_plan.h")).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert re.findall(r"#\s*include", code) == [] and not re.search(r"__\w+__|\bhip[A-Z_]", code)
    assert "potts_pop_plan.h" in open(os.path.join(CSRC, "build.sh")).read()


def test_packing_rule_against_the_host_program_plain_and_sanitized(tmp_path):
    want = _mirror_lines()
    assert _build_and_run(tmp_path, "potts_pop_plan_check", []) == want
    assert _build_and_run(tmp_path, "potts_pop_plan_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]) == want
    # the shapes the timing table names: 16 x 16 packs 16 walkers, 32 x 32 and 8^3 four, 16^3 does not pack
    assert pp.plan_of((16, 16), True, 3, False, 256) == {"route": "k14_pop_pack", "G": 16, "threads": 256, "lds_bytes": 2 * 4 * 256 + 16 * 256}
    assert pp.plan_of((32, 32), True, 8, True, 256)["G"] == 4 and pp.plan_of((8, 8, 8), True, 8, True, 256)["G"] == 4
    assert pp.plan_of((16, 16, 16), True, 3, False, 256) == {"route": "k14_pop_small", "G": 1, "threads": 256, "lds_bytes": 16384}
    assert pp.plan_of((128, 130), True, 3, False, 2)["route"] == "k14_pop_sweep"
    assert pp.plan_of((6, 32), True, 3, True, 70)["G"] == 21 and pp.plan_of((6, 32), True, 3, True, 5)["G"] == 5


def test_header_symbols_prototypes_and_python_surface():
    import tsu
    from tsu import _hip, models
    from tsu.models import potts_population
    with open(os.path.join(ROOT, "include", "tsu_hip.h")) as f:
        top = f.read()
    assert top.index('#include "tsu_hip_potts_pt.h"') < top.index('#include "tsu_hip_potts_pop.h"')
    assert not any(re.search(r"\b" + n + r"\s*\(", re.sub(r"/\*.*?\*/", "", top, flags=re.S)) for n in NEW_SYMBOLS)
    with open(os.path.join(CSRC, "build.sh")) as f:
        build = f.read()
    assert all(n in build for n in ("tsu_hip_potts_pop.h", "potts_pop_kern_dev.h", "potts_pop_plan.h"))
    with open(os.path.join(CSRC, "potts_pop_kern_dev.h")) as f:
        kern = f.read()
    assert re.findall(r"#\s*include\s*[<\"]([^>\"]+)", kern) == ["pop_dev.h", "potts_pop_plan.h", "potts_pt_kern_dev.h"]
    for name in ("k14_pop_pack", "k14_pop_small", "k14_pop_sweep", "k14_pop_measure", "k14_pop_init"):
        assert re.search(r"__global__[^;{]*\b" + name + r"\(", kern), name
    assert len(re.findall(r"\bpd_octet<", kern)) == 3 and "pd_site_thresholds" not in kern and "pd_thresholds" not in kern  # the rule is not forked
    with open(os.path.join(ROOT, "include", "tsu_hip_potts_pop.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tsu_potts_pop_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_hip.POTTS_POP_SIGNATURES)
    lib = _hip.load_library()
    for name in NEW_SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_hip.POTTS_POP_SIGNATURES[name][1]), name
        assert getattr(lib, name).argtypes == _hip.POTTS_POP_SIGNATURES[name][1]
        assert getattr(lib, name).restype is _hip.POTTS_POP_SIGNATURES[name][0]
    routes = [int(re.search(r"#define\s+TSU_POTTS_POP_ROUTE_" + n + r"\s+(\d+)\b", header).group(1)) for n in ("PACK", "SMALL", "SWEEP")]
    assert routes == [0, 1, 2] and _hip.POTTS_POP_ROUTES == pp.ROUTES
    with open(os.path.join(CSRC, "potts_pop_plan.h")) as f:
        rule = f.read()
    for name, value in (("kPopPackThreads", pp.PACK_THREADS), ("kPopPackMaxLanes", pp.PACK_MAX_LANES), ("kPopSmallSites", pp.SMALL_SITES),
                        ("kPopSmallMaxThreads", pp.SMALL_MAX_THREADS)):
        assert int(re.search(name + r"\s*=\s*(\d+)", rule).group(1)) == value, name
    assert re.search(r"kPopPackLds\s*=\s*64 \* 1024", rule) and pp.PACK_LDS == 65536
    with open(os.path.join(CSRC, "pop_dev.h")) as f:
        pop_dev = f.read()
    assert int(re.search(r"kPopMaxWalkers\s*=\s*(\d+)", pop_dev).group(1)) == _hip.POTTS_POP_MAX_WALKERS == 65535
    # no new stream tag; what is shared with the Ising populations and with K13 names nothing of K14
    with open(os.path.join(CSRC, "tsu_common.h")) as f:
        assert sorted(int(v) for v in re.findall(r"TSU_TAG_[A-Z_]+\s*=\s*(\d+)", f.read())) == list(range(13))
    for shared in ("pop_dev.h", "pop_host.h", "potts_pt.hip", "potts_pt_kern_dev.h", "potts_disorder_dev.h", "potts_disorder_kern_dev.h"):
        with open(os.path.join(CSRC, shared)) as f:
            text = f.read()
        assert "k14" not in text and "potts_pop" not in text and "PopWalkers" not in text, shared
    with open(os.path.join(CSRC, "potts_pop.hip")) as f:
        assert "TSU_TAG_" not in re.sub(r"TSU_TAG_(ISING_HI|ISING_LO)\b", "", f.read())
    assert "TSU_TAG_" not in kern.replace("TSU_TAG_INIT", "")
    families = {k: v for k, v in vars(_hip).items() if k.endswith("SIGNATURES") and isinstance(v, dict)}
    for k, v in families.items():
        if k != "POTTS_POP_SIGNATURES":
            assert not set(v) & set(NEW_SYMBOLS), k
    # the Python surface
    names = ("PottsPopulationAnnealing", "PottsPopulationAnnealing3D", "potts_population_annealing_scan", "potts_population_annealing_scan_3d")
    for n in names:
        assert getattr(tsu, n) is getattr(models, n) is getattr(potts_population, n) and n in tsu.__all__ and n in models.__all__
    for cls in (tsu.PottsPopulationAnnealing, tsu.PottsPopulationAnnealing3D):
        params = inspect.signature(cls.__init__).parameters
        assert list(params)[1:4] == ["size", "q", "population"]
        for name in ("betas", "temperatures", "couplings", "site_field", "coupling", "field", "periodic", "seed", "initial", "sweeps_per_step", "initial_sweeps"):
            assert params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert params["initial"].default == "random" and params["sweeps_per_step"].default == 10 and params["initial_sweeps"].default == 0
        for name in ("run", "history", "free_energy", "observables", "family_stats", "spins", "energies", "best", "route", "plan", "launch_count", "close"):
            assert hasattr(cls, name), name
        run = inspect.signature(cls.run).parameters
        assert [run[k].default for k in ("n_steps", "resample", "record")] == [None, True, True]
        assert "device" in cls.__doc__ and "host draw" in cls.__doc__


def test_refusals_come_before_the_device(monkeypatch):
    import tsu
    from tsu import _hip
    from tsu.models import potts_population

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_hip.Context, "default", classmethod(no_device))
    monkeypatch.setattr(_hip, "PottsPopulation", no_device)
    ok2 = (np.zeros((4, 4)), np.zeros((4, 4)))
    ok3 = (np.zeros((4, 4, 4)),) * 3
    open_jr = np.ones((3, 5))
    open_jr[:, -1] = 0
    open_jd = np.ones((3, 5))
    open_jd[-1] = 0
    B = [0.0, 0.5]
    bad2 = [dict(betas=[0.5]), dict(betas=[0.5, 0.5]), dict(betas=[-0.1, 0.5]), dict(betas=[0.0, float("nan")]), dict(betas=None),
            dict(temperatures=[2.0, 1.0]), dict(betas=None, temperatures=[1.0, 2.0]), dict(betas=None, temperatures=[1.0, 0.0]),
            dict(population=1), dict(population=65536), dict(population=2.5), dict(population=True), dict(q=9), dict(q=1),
            dict(initial="up"), dict(initial=3), dict(initial=-2), dict(size=(3, 4)), dict(size=(4, 4, 4)), dict(size=0),
            dict(sweeps_per_step=-1), dict(initial_sweeps=-1),
            dict(couplings=ok2[:1]), dict(couplings=(np.zeros((4, 5)), np.zeros((4, 4)))), dict(couplings=ok2, coupling=2.0),
            dict(site_field=np.zeros((4, 4, 2))), dict(site_field=np.zeros((4, 4, 3)), field=(0.0, 1.0, 0.0)),
            dict(couplings=(np.full((4, 4), float("nan")), ok2[1])), dict(size=(3, 5), periodic=False, couplings=(np.ones((3, 5)), open_jd)),
            dict(size=(3, 5), periodic=False, couplings=(open_jr, np.ones((3, 5)))), dict(seed=2 ** 64 - 1), dict(seed=-1)]
    for kw in bad2:
        args = dict(size=4, q=3, population=8, betas=B)
        args.update(kw)
        with pytest.raises((ValueError, tsu.ConfigurationError)):
            tsu.PottsPopulationAnnealing(**args)
    bad3 = [dict(couplings=ok3[:2]), dict(size=(4, 4)), dict(periodic=(True, True)), dict(size=(3, 4, 4)),
            dict(periodic=(False, True, True), couplings=(ok3[0], ok3[1], np.ones((4, 4, 4)))), dict(betas=[0.5, 0.1]), dict(population=0)]
    for kw in bad3:
        args = dict(size=4, q=3, population=8, betas=B)
        args.update(kw)
        with pytest.raises((ValueError, tsu.ConfigurationError)):
            tsu.PottsPopulationAnnealing3D(**args)
    for cls, kw in ((tsu.PottsPopulationAnnealing, dict(couplings=ok2)),
                    (tsu.PottsPopulationAnnealing, dict(size=(3, 5), periodic=False, couplings=(open_jr, open_jd))),
                    (tsu.PottsPopulationAnnealing, dict(site_field=np.ones((4, 4, 3)), initial=2, population=65535)),
                    (tsu.PottsPopulationAnnealing, dict(betas=None, temperatures=[float("inf"), 2.0, 1.0])),
                    (tsu.PottsPopulationAnnealing3D, dict(couplings=ok3, site_field=np.zeros((4, 4, 4, 3)), seed=2 ** 64 - 8)),
                    (tsu.PottsPopulationAnnealing3D, dict(size=(3, 4, 18), periodic=(False, True, True)))):
        args = dict(size=4, q=3, population=8, betas=B)
        args.update(kw)
        with pytest.raises(AssertionError, match="device was touched"):
            cls(**args)
    with pytest.raises(ValueError):
        potts_population.potts_population_annealing_scan(4, 3, 1, betas=B)
    with pytest.raises(AssertionError, match="device was touched"):
        potts_population.potts_population_annealing_scan(4, 3, 8, betas=B, couplings=ok2)
    with pytest.raises(AssertionError, match="device was touched"):
        potts_population.potts_population_annealing_scan_3d(4, 3, 8, temperatures=[2.0, 1.0], site_field=np.zeros((4, 4, 4, 3)))


@pytest.mark.parametrize("case", pp.ENUM_CASES, ids=lambda c: "x".join(map(str, c[0])) + f"-q{c[1]}")
def test_enumeration_criterion_on_the_reference(case):
    """The criterion of the GPU test on the plain NumPy population annealing, at a quarter of the GPU test's population (R = 256,
    M = 32 generators): ln Z and <E> at every beta within 4 standard errors (spread over the M runs / sqrt(M)) of the sums over all
    q^N states, and the control (no resampling, no sweeps) misses <E> at the last beta by more than that margin."""
    shape, q, per, field, _ = case
    J, h = pp.enum_disorder(case)
    lnZ_x, E_x = pp.exact(pp.state_energies(shape, q, per, J, h), pp.ENUM_BETAS)
    assert lnZ_x[0] == pytest.approx(int(np.prod(shape)) * math.log(q), abs=1e-9)
    runs = [pp.reference_anneal(shape, q, per, J, h, pp.ENUM_BETAS, 256, pp.ENUM_SWEEPS, np.random.default_rng(7000 + m)) for m in range(pp.ENUM_M)]
    worst = pp.criterion([r[0] for r in runs], [r[1] for r in runs], lnZ_x, E_x)
    print("worst ratio", worst)
    assert worst < pp.ENUM_SIGMAS
    ctl = np.array([pp.reference_anneal(shape, q, per, J, h, pp.ENUM_BETAS, 256, 0, np.random.default_rng(7100 + m), resample=False)[1][-1]
                    for m in range(pp.ENUM_M)])
    assert abs(ctl.mean() - E_x[-1]) > pp.ENUM_SIGMAS * ctl.std(ddof=1) / math.sqrt(pp.ENUM_M)

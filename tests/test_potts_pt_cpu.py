"""K13 on the host (no GPU needed): the twin's ladder (tests/helpers/potts_pt_twin.py) against exact enumeration, with the proof that
the check sees the reference's inverted swap rule; the contingency table on hand-made pairs; the new header with its ctypes
prototypes and the build list; the Python refusals ahead of the device; and the assertion that no bit-for-bit GPU case of
tests/test_potts_pt_gpu.py holds a fragile decision."""
import importlib.util
import inspect
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


pt = _load("potts_pt_twin")

NEW_SYMBOLS = ("tsu_potts_pt_create", "tsu_potts_pt_destroy", "tsu_potts_pt_set_disorder", "tsu_potts_pt_set_temperatures",
               "tsu_potts_pt_set_spins", "tsu_potts_pt_get_spins", "tsu_potts_pt_init", "tsu_potts_pt_advance", "tsu_potts_pt_run",
               "tsu_potts_pt_history", "tsu_potts_pt_overlap_tables", "tsu_potts_pt_stats", "tsu_potts_pt_energies", "tsu_potts_pt_route",
               "tsu_potts_pt_launch_count")
K12_SYMBOLS = ("tsu_potts_dis_site_thresholds", "tsu_potts_dis_create", "tsu_potts_dis_destroy", "tsu_potts_dis_set_disorder",
               "tsu_potts_dis_set_spins", "tsu_potts_dis_get_spins", "tsu_potts_dis_fill", "tsu_potts_dis_sweep",
               "tsu_potts_dis_cluster_sweep", "tsu_potts_dis_route", "tsu_potts_dis_measure", "tsu_potts_dis_run", "tsu_potts_dis_record",
               "tsu_potts_dis_launch_count")


def test_fast_chain_equals_the_ladder_built_on_the_shared_twins():
    """tiny_chain (plain Python floats) against Ladders, which only calls potts_disorder_twin.sweep / energy / measure and
    tempering_twin.swap_pass / swap_uniforms: energies per slot, attempts, accepts, round trips and the walkers' places, bit for bit."""
    E = pt.ENUM
    J, h = pt.enum_disorder()
    lad = pt.Ladders(E["shape"], E["q"], E["periodic"], J, h, E["T"], E["seed"], 1, initial=0)
    hist = lad.run(40, 1)
    out, fragile, st = pt.tiny_chain(E["shape"], E["q"], E["periodic"], J, h, E["T"], E["seed"], 40)
    assert fragile == lad.fragile == 0
    assert out.tobytes() == np.ascontiguousarray(hist["E"][:, 0]).tobytes()
    assert (st["attempts"] == lad.attempts[0]).all() and (st["accepts"] == lad.accepts[0]).all() and st["accepts"].sum() > 0
    assert (st["round_trips"] == lad.trips[0]).all() and (st["walker_at_slot"] == lad.walker_at_slot[0]).all()
    assert lad.launches == 40 * (1 + 3 + 1) and lad.sweeps == lad.rounds == 40
    # the recorded integers are the walkers' own
    for i in range(4):
        w = hist["walker"][-1, 0, i]
        n_eq, N = pt.pdt.measure(lad.spins[0][w], E["q"], E["periodic"])
        assert hist["n_eq"][-1, 0, i] == n_eq and (hist["N"][-1, 0, i] == N).all() and N.sum() == 12


def test_twin_ladder_against_enumeration_and_the_inverted_rule_misses():
    """Open 3 x 4, q = 3, Gaussian couplings of both signs and a Gaussian site field, T = 0.5, 0.8, 1.3, 2.0, one swap pass per
    sweep, from colour 0: 500 rounds discarded, 20 000 kept.  <E> at every slot within 4 batch-means errors (32 batches) of the sum
    over all 3^12 states.  The twin gives (E - exact) / error = -0.44, -0.27, -0.29, -0.86 with acceptances 0.43, 0.40, 0.56 and
    about 860 round trips per walker.  The same chain with the reference's E_b - E_a misses by +224, +156, +77 and -680 errors: the
    check sees a wrong swap rule.  No decision of either chain is fragile."""
    E = pt.ENUM
    J, h = pt.enum_disorder()
    assert min(a.min() for a in J) < 0 < max(a.max() for a in J) and h is not None
    exact = pt.exact_energies(E["shape"], E["q"], E["periodic"], J, h, E["T"])
    dev = {}
    for inverted in (False, True):
        out, fragile, st = pt.tiny_chain(E["shape"], E["q"], E["periodic"], J, h, E["T"], E["seed"], E["n_rounds"], E["n_discard"], inverted=inverted)
        err = np.array([pt.batch_means_error(out[:, i]) for i in range(len(E["T"]))])
        dev[inverted] = (out.mean(axis=0) - exact) / err
        print(f"\ninverted={inverted}: <E> = {out.mean(axis=0)}, exact = {exact}, error = {err}, (E - exact) / error = {dev[inverted]}, "
              f"acceptance = {st['accepts'] / st['attempts']}, round trips = {st['round_trips']}")
        assert fragile == 0 and len(out) == E["n_rounds"] - E["n_discard"] and (st["attempts"] == E["n_rounds"]).all()
    assert (np.abs(dev[False]) <= 4.0).all()
    assert (np.abs(dev[True]) > 4.0).any()


def test_contingency_tables_on_hand_made_pairs():
    a = np.array([[0, 1, 2], [2, 1, 0]], np.int8)
    assert (pt.contingency(a, a, 3) == np.diag([2, 2, 2])).all() and pt.overlap(pt.contingency(a, a, 3), 3) == 1.0
    b = (a + 1) % 3  # a permutation of the colours: no site agrees, and the table is a permutation matrix times 2
    C = pt.contingency(a, b, 3)
    assert C.tolist() == [[0, 2, 0], [0, 0, 2], [2, 0, 0]] and pt.overlap(C, 3) == -0.5
    c = np.array([[0, 0, 0], [1, 1, 1]], np.int8)
    C = pt.contingency(a, c, 3)
    assert C.tolist() == [[1, 1, 0], [1, 1, 0], [1, 1, 0]] and C.sum() == 6 and C.dtype == np.int64
    assert (pt.contingency(c, a, 3) == C.T).all() and pt.overlap(C, 3) == (3 * 2 / 6 - 1) / 2
    # 3-D shapes and q = 8 count the same way; the library's Python helper agrees
    from tsu.models import potts_tempering
    rng = np.random.default_rng(3)
    x, y = rng.integers(0, 8, (2, 3, 5)), rng.integers(0, 8, (2, 3, 5))
    C = pt.contingency(x, y, 8)
    assert C.sum() == 30 and np.trace(C) == int((x == y).sum()) and C[x[1, 2, 4], y[1, 2, 4]] >= 1
    assert potts_tempering.potts_overlap(C, 8) == pt.overlap(C, 8)
    assert potts_tempering.potts_overlap(np.stack([C, np.diag([1] * 8)]), 8).tolist() == [pt.overlap(C, 8), 1.0]


def test_gpu_cases_cover_the_issue_and_hold_no_fragile_decision():
    """Every bit-for-bit case of the GPU file, run here first: none holds a fragile site or swap decision, swaps are accepted and
    refused, and the case table has every shape with every q, both fields, both ladder sizes and both ladder counts."""
    cases = pt.cases()
    assert {(c["shape"], c["q"]) for c in cases} == {(s, q) for s, _ in pt.SHAPES for q in (2, 3, 8)}
    for key, want in (("field", {False, True}), ("R", {2, 5}), ("ladders", {1, 2})):
        assert {c[key] for c in cases} == want
        for shape, _ in pt.SHAPES:
            assert {c[key] for c in cases if c["shape"] == shape} == want, (shape, key)
    assert sum(1 for c in cases if c["sweep0"] + pt.N_ROUNDS * pt.INTERVAL > 2 ** 32) == 1
    accepts = attempts = 0
    for c in cases:
        lad = pt.case_twin(c)
        start = [s.copy() for s in lad.spins[0]]
        lad.run(pt.N_ROUNDS, pt.INTERVAL)
        assert lad.fragile == 0, pt.case_id(c)
        assert any((a != b).any() for a, b in zip(start, lad.spins[0])), pt.case_id(c)
        accepts += int(lad.accepts.sum())
        attempts += int(lad.attempts.sum())
    assert 0 < accepts < attempts
    c = pt.LONG
    lad = pt.case_twin(c)
    lad.run(pt.LONG_ROUNDS, pt.LONG_INTERVAL)
    assert lad.fragile == 0 and 0 < lad.accepts.sum() < lad.attempts.sum() == 2 * 129 * pt.LONG_ROUNDS
    assert (lad.walker_at_slot[:, 64:] != np.arange(64, 130)).any()  # the pass moved walkers beyond the first 64 lanes
    for c in pt.BOUNDARY:
        lad = pt.case_twin(c)
        assert lad.small == (c["shape"] == (128, 128))
        lad.run(1, 1)
        assert lad.fragile == 0, c["shape"]


def test_refusals_come_before_the_device(monkeypatch):
    import tsu
    from tsu import _hip
    from tsu.models import potts_tempering

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_hip.Context, "default", classmethod(no_device))
    monkeypatch.setattr(_hip, "PottsTemperingLattice", no_device)
    ok2 = (np.zeros((4, 4)), np.zeros((4, 4)))
    ok3 = (np.zeros((4, 4, 4)),) * 3
    open_jr = np.ones((3, 5))
    open_jr[:, -1] = 0
    open_jd = np.ones((3, 5))
    open_jd[-1] = 0
    T = [1.0, 2.0]
    bad2 = [dict(temperatures=[1.0]), dict(temperatures=np.linspace(1, 2, 257)), dict(temperatures=[1.0, 0.0]), dict(temperatures=[1.0, -2.0]),
            dict(temperatures=[float("nan"), 1.0]), dict(temperatures=[1.0, float("inf")]), dict(ladders=3), dict(ladders=0), dict(q=9), dict(q=1),
            dict(initial="up"), dict(initial=3), dict(initial=-1), dict(size=(3, 4)), dict(size=(4, 4, 4)), dict(size=0),
            dict(couplings=ok2[:1]), dict(couplings=(np.zeros((4, 5)), np.zeros((4, 4)))), dict(couplings=ok2, coupling=2.0),
            dict(site_field=np.zeros((4, 4, 2))), dict(site_field=np.zeros((4, 4, 3)), field=(0.0, 1.0, 0.0)),
            dict(couplings=(np.full((4, 4), float("nan")), ok2[1])), dict(size=(3, 5), periodic=False, couplings=(np.ones((3, 5)), open_jd)),
            dict(size=(3, 5), periodic=False, couplings=(open_jr, np.ones((3, 5)))), dict(seed=2 ** 64 - 1), dict(seed=-1)]
    for kw in bad2:
        args = dict(size=4, q=3, temperatures=T)
        args.update(kw)
        with pytest.raises(tsu.ConfigurationError):
            tsu.PottsTempering(**args)
    bad3 = [dict(couplings=ok3[:2]), dict(size=(4, 4)), dict(periodic=(True, True)), dict(size=(3, 4, 4)),
            dict(periodic=(False, True, True), couplings=(ok3[0], ok3[1], np.ones((4, 4, 4)))), dict(temperatures=[1.0, -1.0]), dict(ladders=3)]
    for kw in bad3:
        args = dict(size=4, q=3, temperatures=T)
        args.update(kw)
        with pytest.raises(tsu.ConfigurationError):
            tsu.PottsTempering3D(**args)
    # what is legal reaches the handle
    for cls, kw in ((tsu.PottsTempering, dict(couplings=ok2)), (tsu.PottsTempering, dict(size=(3, 5), periodic=False, couplings=(open_jr, open_jd))),
                    (tsu.PottsTempering, dict(site_field=np.ones((4, 4, 3)), ladders=2, initial=2)), (tsu.PottsTempering, dict(temperatures=np.linspace(1, 2, 256))),
                    (tsu.PottsTempering3D, dict(couplings=ok3, site_field=np.zeros((4, 4, 4, 3)), seed=2 ** 64 - 2)),
                    (tsu.PottsTempering3D, dict(size=(3, 4, 18), periodic=(False, True, True)))):
        args = dict(size=4, q=3, temperatures=T)
        args.update(kw)
        with pytest.raises(AssertionError, match="device was touched"):
            cls(**args)
    for kw in (dict(replicas=3), dict(n_equilibrate=15, measure_every=10), dict(n_measure=0)):
        with pytest.raises(ValueError):
            potts_tempering.potts_tempering_scan(4, 3, T, couplings=ok2, **kw)
    with pytest.raises(tsu.ConfigurationError):
        potts_tempering.potts_tempering_scan(4, 3, [1.0, -1.0], couplings=ok2)
    with pytest.raises(AssertionError, match="device was touched"):
        potts_tempering.potts_tempering_scan(4, 3, T, couplings=ok2, replicas=2)
    with pytest.raises(AssertionError, match="device was touched"):
        potts_tempering.potts_tempering_scan_3d(4, 3, T, site_field=np.zeros((4, 4, 4, 3)))


def test_header_symbols_prototypes_and_python_surface():
    import tsu
    from tsu import _hip, models
    from tsu.models import potts_tempering
    with open(os.path.join(ROOT, "include", "tsu_hip.h")) as f:
        top = f.read()
    assert re.search(r'^#include "tsu_hip_potts_pt.h"', top, flags=re.M)
    assert top.index('#include "tsu_hip_potts_disorder.h"') < top.index('#include "tsu_hip_potts_pt.h"')
    assert not any(re.search(r"\b" + n + r"\s*\(", re.sub(r"/\*.*?\*/", "", top, flags=re.S)) for n in NEW_SYMBOLS)
    with open(os.path.join(CSRC, "build.sh")) as f:
        build = f.read()
    assert "tsu_hip_potts_pt.h" in build and "potts_pt_kern_dev.h" in build
    assert os.path.exists(os.path.join(CSRC, "potts_pt.hip"))
    with open(os.path.join(CSRC, "potts_pt_kern_dev.h")) as f:
        kern = f.read()
    assert re.findall(r"#\s*include\s*[<\"]([^>\"]+)", kern) == ["potts_disorder_kern_dev.h", "pt_dev.h"]
    for name in ("k13_pt_small", "k13_pt_sweep", "k13_pt_measure", "k13_pt_final", "k13_pt_table", "k13_pt_gather"):
        assert re.search(r"__global__[^;{]*\b" + name + r"\(", kern), name
    with open(os.path.join(ROOT, "include", "tsu_hip_potts_pt.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tsu_potts_pt_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_hip.POTTS_PT_SIGNATURES)
    assert not re.search(r"\btsu_potts_dis_[a-z0-9_]+\s*\(", header)
    lib = _hip.load_library()
    for name in NEW_SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_hip.POTTS_PT_SIGNATURES[name][1]), name
        assert getattr(lib, name).argtypes == _hip.POTTS_PT_SIGNATURES[name][1]
        assert getattr(lib, name).restype is _hip.POTTS_PT_SIGNATURES[name][0]
    routes = [int(re.search(r"#define\s+TSU_POTTS_PT_ROUTE_" + n + r"\s+(\d+)\b", header).group(1)) for n in ("SMALL", "SWEEP")]
    assert routes == [0, 1] and _hip.POTTS_PT_ROUTES == ("k13_pt_small", "k13_pt_sweep")
    with open(os.path.join(CSRC, "pt_dev.h")) as f:
        assert int(re.search(r"kPtMaxTemps\s*=\s*(\d+)", f.read()).group(1)) == _hip.POTTS_PT_MAX_TEMPS == 256
    # no new stream tag: tsu_common.h's enum stays 0 .. 12, and the new unit names only the sweeps' two (the swap's is pt_dev.h's)
    with open(os.path.join(CSRC, "tsu_common.h")) as f:
        assert sorted(int(v) for v in re.findall(r"TSU_TAG_[A-Z_]+\s*=\s*(\d+)", f.read())) == list(range(13))
    with open(os.path.join(CSRC, "potts_pt.hip")) as f:
        assert "TSU_TAG_" not in re.sub(r"TSU_TAG_(ISING_HI|ISING_LO)\b", "", f.read())
    assert "TSU_TAG_" not in kern
    # a family of its own, disjoint from every other one
    families = {k: v for k, v in vars(_hip).items() if k.endswith("SIGNATURES") and isinstance(v, dict)}
    assert "POTTS_PT_SIGNATURES" in families
    for k, v in families.items():
        if k != "POTTS_PT_SIGNATURES":
            assert not set(v) & set(NEW_SYMBOLS), k
    # K12's header still declares exactly its 14 symbols
    with open(os.path.join(ROOT, "include", "tsu_hip_potts_disorder.h")) as f:
        k12 = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(tsu_potts_dis_[a-z0-9_]+)\s*\(", k12))) == sorted(K12_SYMBOLS) == sorted(_hip.POTTS_DISORDER_SIGNATURES)
    assert len(K12_SYMBOLS) == 14 and "tsu_potts_pt_" not in k12
    # the Python surface
    for n in ("PottsTempering", "PottsTempering3D", "potts_tempering_scan", "potts_tempering_scan_3d"):
        assert getattr(tsu, n) is getattr(models, n) is getattr(potts_tempering, n) and n in tsu.__all__ and n in models.__all__
    for cls in (tsu.PottsTempering, tsu.PottsTempering3D):
        assert issubclass(cls, potts_tempering._PottsTempering)
        params = inspect.signature(cls.__init__).parameters
        assert list(params)[1:4] == ["size", "q", "temperatures"]
        for name in ("couplings", "site_field", "coupling", "field", "periodic", "seed", "initial", "ladders"):
            assert params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert params["initial"].default == "random" and params["ladders"].default == 1 and params["coupling"].default == 1.0
        for name in ("run", "history", "swap_acceptance", "round_trips", "walker_at_slot", "energies", "spins", "route", "launch_count", "close"):
            assert hasattr(cls, name), name
        run = inspect.signature(cls.run).parameters
        assert [run[k].default for k in ("swap_interval", "swap", "record")] == [10, True, True]
    for fn in (potts_tempering.potts_tempering_scan, potts_tempering.potts_tempering_scan_3d):
        params = inspect.signature(fn).parameters
        assert params["couplings"].kind is params["site_field"].kind is params["replicas"].kind is inspect.Parameter.KEYWORD_ONLY
        assert "seed + g" in fn.__doc__

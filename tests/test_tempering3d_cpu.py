"""K8 parallel tempering on the host: the NumPy twin (tests/helpers/tempering3d_twin.py) against lattice3d_twin's sweeps without
swaps and against the 2-D ladders' twin on a one-layer lattice, its initial draw against the oracle's randomize, validation before
the device is touched, and the new C-ABI symbols (no GPU needed)."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

from oracle import oracle as ora

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_spec = importlib.util.spec_from_file_location("tempering3d_twin", os.path.join(HERE, "helpers", "tempering3d_twin.py"))
twin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(twin)
twin2 = twin.tempering_twin
ltwin = twin.lattice3d_twin

PT3_SYMBOLS = ["tsu_pt3d_create", "tsu_pt3d_destroy", "tsu_pt3d_set_disorder", "tsu_pt3d_set_temperatures", "tsu_pt3d_init",
               "tsu_pt3d_run", "tsu_pt3d_history", "tsu_pt3d_stats", "tsu_pt3d_energies", "tsu_pt3d_get_spins", "tsu_pt3d_set_spins",
               "tsu_pt3d_launch_count"]


def _disorder(shape, periodic, seed):
    rng = np.random.default_rng(seed)
    jr, jd, jl, h = (rng.normal(size=shape).astype(np.float32) for _ in range(4))
    pz, pr, pc = ltwin.axes(periodic)
    if not pc:
        jr[:, :, -1] = 0.0
    if not pr:
        jd[:, -1, :] = 0.0
    if not pz:
        jl[-1, :, :] = 0.0
    return jr, jd, jl, h


def test_twin_has_the_shared_swap_pass():
    """The issue's rule: no second statement of the swap pass, the uniforms or the bookkeeping."""
    assert twin.swap_pass is twin2.swap_pass and twin.swap_uniforms is twin2.swap_uniforms and twin.arrive is twin2.arrive
    assert twin.sweep is ltwin.sweep and twin.energy is ltwin.energy and twin.overlap is ltwin.overlap


@pytest.mark.parametrize("shape,seed", [((3, 5, 37), 7), ((2, 4, 130), 2 ** 40 + 5), ((1, 6, 300), 99)])
def test_initial_draw_is_randomize_of_the_global_rows(shape, seed):
    D, R, C = shape
    got = twin.initial_spins(shape, seed, 3)
    for g in range(3):
        assert (got[g].reshape(D * R, C) == ora.ising2d_randomize(D * R, C, seed + g)).all(), g
    assert (twin.initial_spins(shape, seed, 2, -1)[1] == -1).all()


@pytest.mark.parametrize("shape,periodic,ladders", [((4, 4, 6), True, 2), ((3, 5, 9), False, 1), ((4, 3, 20), (True, False, False), 2)])
def test_without_swaps_every_walker_is_a_k8_lattice(shape, periodic, ladders):
    """swap=False: walker w of ladder k is model k R + w of temperature_scan_3d, swept by lattice3d_twin.sweep."""
    Ts = [0.5, 1.1, 2.3]
    R, seed = len(Ts), 31
    dis = _disorder(shape, periodic, 5)
    start = twin.initial_spins(shape, seed, ladders * R)
    tw = twin.Ladders([start[k * R:(k + 1) * R] for k in range(ladders)], periodic, dis, Ts, seed)
    h1 = tw.run(2, 3, False, True)
    h2 = tw.run(1, 2, False, False)
    assert h2["E"].shape == (0, ladders, R) and tw.sweeps == 8 and tw.rounds == 3
    assert (tw.walker_at_slot == np.arange(R)).all() and tw.attempts.sum() == 0 and tw.trips.sum() == 0
    for k in range(ladders):
        for w in range(R):
            g = k * R + w
            want = ltwin.sweep(start[g], periodic, *dis, Ts[w], 8, seed + g, 0, 0)
            assert (tw.spins[k][w] == want).all(), (k, w)
            mid = ltwin.sweep(start[g], periodic, *dis, Ts[w], 6, seed + g, 0, 0)
            assert h1["E"][1, k, w] == ltwin.energy(mid, periodic, *dis) and h1["M"][1, k, w] == mid.sum()
    if ladders == 2:
        mid = [ltwin.sweep(start[k * R], periodic, *dis, Ts[0], 6, seed + k * R, 0, 0) for k in range(2)]
        assert h1["q"][1, 0] == ltwin.overlap(*mid)


@pytest.mark.parametrize("rows,cols,periodic,ladders", [(6, 10, True, 2), (5, 37, False, 1), (4, 8, True, 1)])
def test_one_layer_ladder_is_the_2d_ladder(rows, cols, periodic, ladders):
    """D = 1 with an open z axis, fed the same energies: the 3-D twin reproduces tempering_twin.Ladders in spins, tables, counters."""
    Ts = [0.4, 0.8, 1.3, 2.0]
    R, seed = len(Ts), 77
    rng = np.random.default_rng(rows)
    jr, jd, h = (rng.normal(size=(rows, cols)).astype(np.float32) for _ in range(3))
    if not periodic:
        jr[:, -1] = 0.0
        jd[-1, :] = 0.0
    shape = (1, rows, cols)
    start = twin.initial_spins(shape, seed, ladders * R)
    two = twin2.Ladders([[s.reshape(rows, cols) for s in start[k * R:(k + 1) * R]] for k in range(ladders)], periodic, (jr, jd, h),
                        Ts, seed)
    three = twin.Ladders([start[k * R:(k + 1) * R] for k in range(ladders)], (False, periodic, periodic),
                         (jr.reshape(shape), jd.reshape(shape), np.zeros(shape, np.float32), h.reshape(shape)), Ts, seed)
    dt = twin2.disorder_twin
    for n_rounds, interval in ((6, 2), (5, 1)):
        fed = []

        def energies(j, k):  # the 2-D twin's float64 energies of its own walkers, recorded and fed to both
            while len(fed) <= j:
                fed.append({})
            if k not in fed[j]:
                fed[j][k] = np.array([dt.energy(s, periodic, jr, jd, h) for s in two.spins[k]])
            return fed[j][k]
        a = two.run(n_rounds, interval, True, True, energies)
        b = three.run(n_rounds, interval, True, True, lambda j, k: fed[j][k])
        for key in ("E", "M", "walker"):
            assert np.array_equal(a[key], b[key]), key
        if ladders == 2:
            assert np.array_equal(a["q"], b["q"])
        for name in ("walker_at_slot", "flags", "trips", "attempts", "accepts"):
            assert np.array_equal(getattr(two, name), getattr(three, name)), name
        assert (two.sweeps, two.rounds) == (three.sweeps, three.rounds)
        for k in range(ladders):
            for w in range(R):
                assert (three.spins[k][w].reshape(rows, cols) == two.spins[k][w]).all(), (k, w)
    assert two.accepts.sum() > 0


# ---------------------------------------------------------------- validation before the device is touched
@pytest.fixture
def no_device(monkeypatch):
    from tsu import _hip

    def boom(*a, **k):
        raise AssertionError("the device was touched before validation")
    monkeypatch.setattr(_hip, "TemperingLattice3D", boom)
    monkeypatch.setattr(_hip, "Lattice3D", boom)
    return _hip


S = (4, 6, 8)


def _arrays(shape, periodic=True):
    return ltwin.uniform_disorder(shape, periodic, 1.0, 0.0)[:3]


BAD = [
    dict(size=(4, 6)),                                                          # bad sizes
    dict(size=(4, 0, 8)),
    dict(size=(4, 6, 8, 2)),
    dict(size=(5, 6, 8)),                                                       # an odd periodic axis
    dict(size=(4, 2, 8)),                                                       # a short periodic axis
    dict(size=(4, 6, 7), periodic=(False, False, True)),
    dict(couplings=_arrays(S), periodic=(True, True, False)),                   # a nonzero last slice on an open axis
    dict(couplings=_arrays(S), periodic=(True, False, True)),
    dict(couplings=_arrays(S), periodic=(False, True, True)),
    dict(couplings=(np.full(S, np.nan),) + _arrays(S)[1:]),                     # non-finite disorder
    dict(couplings=_arrays(S)[:2] + (np.full(S, np.inf),)),
    dict(field=np.full(S, -np.inf)),
    dict(field=np.full(S, 1e300)),
    dict(couplings=_arrays((4, 6, 6))),
    dict(couplings=_arrays(S)[:2]),
    dict(couplings=_arrays(S), coupling=2.0),
    dict(field=np.zeros(S), external_field=0.5),
    dict(temperatures=[1.0]),                                                   # 1 or 257 temperatures
    dict(temperatures=np.linspace(0.5, 2.0, 257)),
    dict(temperatures=[1.0, 0.0]),                                              # a non-positive temperature
    dict(temperatures=[1.0, -2.0]),
    dict(temperatures=[1.0, np.nan]),
    dict(temperatures=[1.0, np.inf]),
    dict(ladders=3),
    dict(ladders=0),
    dict(initial="sideways"),
    dict(periodic=(True, True)),
]


@pytest.mark.parametrize("kw", BAD)
def test_tempering_validation_precedes_device(no_device, kw):
    from tsu.models.ising import LatticeTempering3D
    args = dict(size=S, temperatures=[0.5, 1.0, 2.0], seed=1)
    args.update(kw)
    with pytest.raises(ValueError):
        LatticeTempering3D(args.pop("size"), args.pop("temperatures"), **args)


def test_periodic_axis_rule_keeps_k8s_error_type(no_device):
    """The periodic-axis rule is refused as a ValueError (above) that is also K8's UnsupportedError, as IsingModel3D raises it."""
    from tsu.models.ising import LatticeTempering3D, tempering_scan_3d
    with pytest.raises(no_device.UnsupportedError, match="even length"):
        LatticeTempering3D((5, 6, 8), [1.0, 2.0], seed=1)
    with pytest.raises(no_device.UnsupportedError, match="even length"):
        tempering_scan_3d((4, 6, 2), [1.0, 2.0], periodic=(False, False, True))


def test_tempering_scan_validation_precedes_device(no_device):
    from tsu.models.ising import tempering_scan_3d
    jr, jd, jl = _arrays(S)
    with pytest.raises(ValueError):
        tempering_scan_3d(S, [1.0, 2.0], couplings=(jr, jd, jl), replicas=3)
    with pytest.raises(ValueError, match="multiple of measure_every"):
        tempering_scan_3d(S, [1.0, 2.0], couplings=(jr, jd, jl), n_equilibrate=15, measure_every=10)
    with pytest.raises(ValueError, match="multiple of measure_every"):
        tempering_scan_3d(S, [1.0, 2.0], n_equilibrate=10, measure_every=0)
    with pytest.raises(ValueError):
        tempering_scan_3d(S, [1.0, 2.0], field=np.zeros((4, 8, 6)))
    with pytest.raises(ValueError):
        tempering_scan_3d(S, [1.0, 2.0], couplings=(jr, jd, jl), coupling=2.0)
    with pytest.raises(ValueError):
        tempering_scan_3d(S, [1.0, 0.0])
    with pytest.raises(ValueError):
        tempering_scan_3d(S, [1.0], n_equilibrate=10)
    with pytest.raises(ValueError):
        tempering_scan_3d((5, 6, 8), [1.0, 2.0])
    with pytest.raises(ValueError):
        tempering_scan_3d(S, [1.0, 2.0], couplings=(jr, jd, jl), periodic=(True, False, True))
    with pytest.raises(ValueError):
        tempering_scan_3d(S, [1.0, 2.0], initial="sideways")


def test_symbols_in_header_and_library():
    from tsu import _hip
    header = open(os.path.join(ROOT, "include", "tsu_hip.h")).read()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for n in PT3_SYMBOLS:
        assert re.search(rf"\b{n}\s*\(", header), n
        assert hasattr(lib, n), n
        assert n in _hip.SIGNATURES, n
        # the ctypes signature has the header's arity and the 2-D counterpart's types after the shape arguments
        proto = re.search(rf"\b{n}\s*\(([^;]*)\)\s*;", header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_hip.SIGNATURES[n][1]), n
        two = _hip.SIGNATURES[n.replace("pt3d", "pt2d")][1]
        if n == "tsu_pt3d_create":
            assert _hip.SIGNATURES[n][1] == two[:1] + [ctypes.c_int] + two[1:]
        elif n == "tsu_pt3d_set_disorder":
            assert _hip.SIGNATURES[n][1] == two + two[-1:]
        else:
            assert _hip.SIGNATURES[n][1] == two, n
    assert hasattr(_hip, "TemperingLattice3D") and hasattr(_hip.TemperingLattice3D, "close")
    import tsu
    from tsu import models
    for mod in (models, tsu):
        assert "LatticeTempering3D" in mod.__all__ and "tempering_scan_3d" in mod.__all__
        assert hasattr(mod, "LatticeTempering3D") and hasattr(mod, "tempering_scan_3d")


def test_swap_kernel_is_defined_once():
    """Both handle types run the one ladder core: over all of csrc the swap kernel is launched once, in pt_host.h, and the swap,
    pt_energy_final and pt_overlap kernels are defined once each; neither source file defines a swap kernel of its own."""
    csrc = os.path.join(ROOT, "tsu-emulator_amd", "csrc")
    pat = re.compile(r"__global__[^;{]*\bk\d_pt_swap\b")
    assert len(pat.findall(open(os.path.join(csrc, "pt_dev.h")).read())) == 1
    for name in ("ising2d_disorder.hip", "ising3d.hip", "ising2d_icm.hip"):
        src = open(os.path.join(csrc, name)).read()
        assert not pat.search(src), name
    sources = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))}
    launches = {f: len(re.findall(r"\bk\d_pt_swap\s*<<<", s)) for f, s in sources.items()}
    assert {f: n for f, n in launches.items() if n} == {"pt_host.h": 1}
    for kernel in (r"k\d_pt_swap", r"(?:k\d_)?pt_energy_final", r"(?:k\d_)?pt_overlap"):
        defs = re.compile(rf"__global__[^;{{]*\b{kernel}\s*\(")
        assert sum(len(defs.findall(s)) for s in sources.values()) == 1, kernel
    build = open(os.path.join(csrc, "build.sh")).read()
    for header in ("pt_dev.h", "pt_host.h", "reduce_dev.h"):
        assert header in build, header

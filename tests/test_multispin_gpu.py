"""K9 on the GPU: every spin of every sample of a multispin-coded glass against IsingModel3D (IsingModel2D for one layer) run on that
sample with the plane's seed, on both routes; energies, sums of spins, q and q_l as exact integers; pad bits, ties, launch counts
and the scan."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


twin = _load("multispin_twin")
lat3 = twin.lat3

# name -> (shape, periodic, S, temperatures, replicas, dims)
CASES = {
    "cube4_one_sample": ((4, 4, 4), True, 1, (1.3,), 1, 3),
    "open_partial_word": ((3, 5, 18), False, 65, (1.1,), 1, 3),          # odd neighbour counts, a partial octet, a partial word
    "one_layer_2d": ((1, 6, 34), (False, True, True), 64, (1.7,), 1, 2),  # against IsingModel2D
    "mixed_three_slots": ((4, 6, 40), (True, False, True), 130, (0.5, 1.1, 2.0), 2, 3),
    "nine_octets_per_row": ((4, 4, 132), True, 64, (0.9,), 1, 3),         # more than eight octets per row
}
SEED = (3 << 32) | 17
SPLIT = (3, 7)  # 10 sweeps in two calls: the second starts at sweep0 = 3
_reference = {}
_couplings = {}


def couplings_of(name):
    from tsu.models import edwards_anderson_samples
    if name not in _couplings:
        shape, periodic, S, _, _, dims = CASES[name]
        if dims == 2:
            _couplings[name] = edwards_anderson_samples(shape[1:], S, kind="bimodal", seed=21, dims=2, periodic=periodic[1:])
        else:
            _couplings[name] = edwards_anderson_samples(shape, S, kind="bimodal", seed=21, periodic=periodic)
    return _couplings[name]


def reference(name):
    """Spins and integers of every (slot, replica, sample) from the single-lattice models, computed once per case."""
    from tsu.models import IsingModel2D, IsingModel3D
    from tsu.models.ising import lattice_bond_count
    if name in _reference:
        return _reference[name]
    shape, periodic, S, Ts, A, dims = CASES[name]
    j = couplings_of(name)
    nT, N = len(Ts), int(np.prod(shape))
    out = {"spins": np.zeros((nT, A, S) + shape, np.int8), "E": np.zeros((nT, A, S)), "M": np.zeros((nT, A, S), np.int64),
           "q": np.zeros((nT, S), np.int64), "ql": np.zeros((nT, S), np.int64), "nb": lattice_bond_count(shape, periodic)}
    for t, T in enumerate(Ts):
        for s in range(S):
            pair = []
            for a in range(A):
                seed = SEED + a * nT + t
                if dims == 2:
                    m = IsingModel2D(shape[1:], temperature=T, periodic=True, seed=seed, couplings=(j[0][s], j[1][s]))
                else:
                    m = IsingModel3D(shape, temperature=T, periodic=periodic, seed=seed, couplings=tuple(x[s] for x in j))
                for n in SPLIT:
                    m.gibbs_update(n)
                out["spins"][t, a, s] = m.spins.reshape(shape)
                out["E"][t, a, s] = m.energy()
                out["M"][t, a, s] = int(out["spins"][t, a, s].sum(dtype=np.int64))
                assert out["M"][t, a, s] / N == m.magnetization()
                pair.append(m)
            if A == 2:
                out["q"][t, s] = pair[0]._lat.overlap(pair[1]._lat)
                L, nb = pair[0]._lat.link_overlap(pair[1]._lat)
                assert nb == out["nb"]
                out["ql"][t, s] = L
                assert pair[0].overlap(pair[1]) == out["q"][t, s] / N and pair[0].link_overlap(pair[1]) == L / nb
            for m in pair:
                m._lat.close()
    _reference[name] = out
    return out


def build(name, route, **kw):
    from tsu.models import MultispinGlass3D
    shape, periodic, S, Ts, A, _ = CASES[name]
    return MultispinGlass3D(shape, Ts, couplings=couplings_of(name), periodic=periodic, replicas=A, seed=SEED, route=route, **kw)


@pytest.mark.parametrize("route", ["small", "hbm"])
@pytest.mark.parametrize("name", list(CASES))
def test_every_bit_is_the_single_lattice(name, route):
    shape, periodic, S, Ts, A, _ = CASES[name]
    ref = reference(name)
    g = build(name, route)
    try:
        assert g.route == route and g.n_samples == S
        for n in SPLIT:
            g.sweep(n)
        assert g.sweep_count == sum(SPLIT)
        got = g.spin_array()
        assert got.shape == ref["spins"].shape
        assert (got == ref["spins"]).all(), f"{int((got != ref['spins']).sum())} spins differ"
        unsat, ssum, q, ql = g._msc.measure()
        assert unsat.dtype == np.int64 and unsat.shape == ssum.shape == (len(Ts), A, S)
        assert (2 * unsat - ref["nb"] == ref["E"]).all() and (ssum == ref["M"]).all()
        E, M = g.energies(), g.magnetizations()
        if A == 2:
            assert q.shape == ql.shape == (len(Ts), S)
            assert (q == ref["q"]).all() and (ql == ref["ql"]).all()
            assert (E == ref["E"]).all() and (M == ref["M"] / g.n_spins).all()
            assert (g.overlaps() == ref["q"] / g.n_spins).all() and (g.link_overlaps() == ref["ql"] / ref["nb"]).all()
        else:
            assert q is None and ql is None
            assert (E == ref["E"][:, 0]).all() and (M == ref["M"][:, 0] / g.n_spins).all()
            with pytest.raises(ValueError, match="replicas=2"):
                g.overlaps()
        s, t = S - 1, len(Ts) - 1
        assert (g.spins(s, t, A - 1) == ref["spins"][t, A - 1, s]).all()
    finally:
        g.close()


def test_the_two_routes_give_equal_bits():
    from tsu.models import MultispinGlass3D, edwards_anderson_samples
    j = edwards_anderson_samples(8, 70, kind="bimodal", seed=5)
    planes = []
    for route in ("small", "hbm", None):
        g = MultispinGlass3D(8, [0.8, 1.6], couplings=j, replicas=2, seed=9, route=route)
        assert g.route == (route or "small")
        g.sweep(4).sweep(5)
        planes.append(g._msc.get_planes())
        g.close()
    assert planes[0].shape == (2, 2, 2, 8, 8, 8)
    assert (planes[0] == planes[1]).all() and (planes[0] == planes[2]).all()
    assert len(np.unique(planes[0])) > 1000


def test_the_small_route_refuses_what_does_not_fit():
    from tsu import _hip
    from tsu.models import MultispinGlass3D, edwards_anderson_samples
    shape = (4, 4, 1024)  # 16384 sites
    j = edwards_anderson_samples(shape, 1, kind="bimodal", seed=5)
    with pytest.raises(_hip.UnsupportedError, match="small route"):
        MultispinGlass3D(shape, [1.0], couplings=j, seed=1, route="small")
    g = MultispinGlass3D(shape, [1.0], couplings=j, seed=1)
    assert g.route == "hbm"
    g.close()


def test_pad_bits_never_leak():
    """S = 65: every output has 65 columns, and they equal the first 65 of S = 128 on the same samples, whose word 1 is full."""
    from tsu.models import MultispinGlass3D, edwards_anderson_samples
    shape, Ts = (4, 4, 6), [0.7, 1.9]
    j = edwards_anderson_samples(shape, 128, kind="bimodal", seed=6)
    outs = []
    for S in (65, 128):
        g = MultispinGlass3D(shape, Ts, couplings=tuple(a[:S] for a in j), replicas=2, seed=4)
        g.sweep(6)
        outs.append((g.energies(), g.magnetizations(), g.overlaps(), g.link_overlaps(), g.spin_array()))
        g.close()
    e, m, q, ql, sp = outs[0]
    assert e.shape == m.shape == (2, 2, 65) and q.shape == ql.shape == (2, 65) and sp.shape == (2, 2, 65) + shape
    assert (e == outs[1][0][..., :65]).all() and (m == outs[1][1][..., :65]).all()
    assert (q == outs[1][2][..., :65]).all() and (ql == outs[1][3][..., :65]).all()
    assert (sp == outs[1][4][:, :, :65]).all()


TIE_SEED = 3  # fixed after a check on the CPU (test_multispin_cpu.test_ties_take_the_low_half): the construction below finds a site


@pytest.mark.parametrize("route", ["small", "hbm"])
def test_a_tie_on_the_top_half_draws_the_low_half(route):
    """All spins up, T = 2 f / logit(u / 2^32) from the uniform of a colour-0 site of sweep 0 with f != 0: that decision sits on its
    threshold.  The twin confirms on the CPU that the run holds a hi16 tie; the GPU must then still equal the single lattice."""
    from tsu.models import IsingModel3D, MultispinGlass3D, edwards_anderson_samples
    shape, S = (4, 4, 4), 3
    j = edwards_anderson_samples(shape, S, kind="bimodal", seed=1)
    spins = np.ones((S,) + shape, np.int8)
    f = lat3.local_field(spins[0], True, *lat3.as_disorder(shape, j[0][0], j[1][0], j[2][0]))
    u = lat3.site_uniforms(shape, 0, TIE_SEED).astype(np.float64) / 4294967296.0
    logit = np.log(u) - np.log1p(-u)
    ok = (lat3.colours(shape) == 0) & (f != 0) & (f * logit > 0)
    assert ok.any()
    z, r, c = np.argwhere(ok)[0]
    T = float(2.0 * f[z, r, c] / logit[z, r, c])
    assert twin.sample_ties(spins, True, j, T, 2, TIE_SEED) >= 1
    g = MultispinGlass3D(shape, [T], couplings=j, seeds=[[TIE_SEED]], initial="up", route=route)
    g.sweep(2)
    got = g.spin_array()[0, 0]
    g.close()
    assert (got == twin.reference_sweep(spins, True, j, T, 2, TIE_SEED)).all()
    for s in range(S):
        m = IsingModel3D(shape, temperature=T, seed=TIE_SEED, initial="up", couplings=tuple(a[s] for a in j))
        m.gibbs_update(2)
        assert (got[s] == m.spins).all()
        m._lat.close()


def test_launch_counts():
    """The small route launches once per sweep(n) call, the HBM route 2 n times, whatever the number of planes."""
    from tsu.models import MultispinGlass3D, edwards_anderson_samples
    shape = (4, 4, 6)
    for S, Ts, A in ((3, [1.0], 1), (130, [0.6, 1.0, 1.4], 2)):
        j = edwards_anderson_samples(shape, S, kind="bimodal", seed=6)
        for route, per_call in (("small", lambda n: 1), ("hbm", lambda n: 2 * n)):
            g = MultispinGlass3D(shape, Ts, couplings=j, replicas=A, seed=2, route=route)
            assert g.launch_count == 0
            g.sweep(3)
            assert g.launch_count == per_call(3)
            g.sweep(5)
            assert g.launch_count == per_call(3) + per_call(5)
            g.energies()
            g.sweep(0)
            assert g.launch_count == per_call(3) + per_call(5) and g.sweep_count == 8
            g.close()


def test_set_spins_round_trip():
    from tsu.models import MultispinGlass3D, edwards_anderson_samples
    shape = (4, 4, 6)
    j = edwards_anderson_samples(shape, 66, kind="bimodal", seed=6)
    g = MultispinGlass3D(shape, [1.0, 2.0], couplings=j, replicas=2, seed=2, initial="down")
    v = np.random.default_rng(1).choice(np.array([-1, 1], np.int8), size=shape)
    g.set_spins(65, 1, v, replica=1)
    all_spins = g.spin_array()
    assert (all_spins[1, 1, 65] == v).all() and (g.spins(65, 1, 1) == v).all()
    all_spins[1, 1, 65] = -1
    assert (all_spins == -1).all()
    assert (g.magnetizations()[1, 1, 65] == v.sum() / v.size) and (g.magnetizations()[0] == -1.0).all()
    g.close()


def test_scan_returns_the_documented_keys():
    from tsu.models import edwards_anderson_samples, multispin_scan_3d
    from tsu.models.ising import lattice_bond_count
    shape, S, Ts = (4, 4, 4), 64, [0.8, 1.5, 3.0]
    j = edwards_anderson_samples(shape, S, kind="bimodal", seed=8)
    res = multispin_scan_3d(shape, Ts, couplings=j, n_equilibrate=20, n_measure=10, measure_every=2, replicas=2, seed=1)
    keys = ("energy", "magnetization", "overlap", "overlap_sq", "overlap_4", "link_overlap")
    for k in keys:
        assert res[k].shape == (S, len(Ts)), k
    assert (res["temperatures"] == np.asarray(Ts)).all()
    avg = res["average"]
    for k in ("energy", "magnetization", "overlap", "overlap_sq", "link_overlap"):
        assert avg[k].shape == (len(Ts),) and avg[k + "_err"].shape == (len(Ts),) and np.isfinite(avg[k]).all(), k
    assert avg["binder"].shape == (len(Ts),)
    assert ((avg["overlap_sq"] >= 0) & (avg["overlap_sq"] <= 1)).all()
    assert ((res["overlap_sq"] >= 0) & (res["overlap_sq"] <= 1)).all() and (np.abs(res["link_overlap"]) <= 1).all()
    per_bond = res["energy"] * 64 / lattice_bond_count(shape, True)
    assert ((per_bond >= -1) & (per_bond <= 0)).all()
    assert (np.diff(avg["energy"]) > 0).all()  # colder is lower

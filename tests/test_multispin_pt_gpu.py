"""K9 tempering on the GPU: without swaps the plain glass; with swaps every word, row and counter against the NumPy twin driving a
second, plain handle, and against IsingModel3D models exchanged through their spins setter; forced passes in which a
configuration climbs the whole ladder in one pass; a ladder of 256 temperatures; equilibrium against full enumeration; launch
counts and continuation."""
import importlib.util
import math
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


twin = _load("multispin_pt_twin")
msc = twin.msc

# name -> (shape, periodic, dims)
CASES = {
    "cube": ((4, 4, 6), True, 3),
    "one_layer": ((1, 6, 34), (False, True, True), 2),
    "open_rows": ((4, 5, 18), (True, False, True), 3),  # an odd open axis, a partial octet
}
S = 70  # two words, 58 pad bits
TS = (0.6, 0.9, 1.3, 1.8, 2.5)
A = 2
SEED = (5 << 32) | 23
SWAP_SEED = (9 << 32) | 4
ROUNDS, K = 6, 2
_couplings = {}
_twin_run = {}


def couplings_of(name, n_samples=S):
    from tsu.models import edwards_anderson_samples
    if (name, n_samples) not in _couplings:
        shape, periodic, dims = CASES[name]
        if dims == 2:
            j = edwards_anderson_samples(shape[1:], n_samples, kind="bimodal", seed=31, dims=2, periodic=periodic[1:])
        else:
            j = edwards_anderson_samples(shape, n_samples, kind="bimodal", seed=31, periodic=periodic)
        _couplings[(name, n_samples)] = j
    return _couplings[(name, n_samples)]


def tempering(name, route, **kw):
    from tsu.models import MultispinTempering3D
    shape, periodic, _ = CASES[name]
    kw.setdefault("swap_seed", SWAP_SEED)
    return MultispinTempering3D(shape, TS, couplings=couplings_of(name), periodic=periodic, replicas=A, seed=SEED, route=route, **kw)


def plain(name, route=None):
    from tsu.models import MultispinGlass3D
    shape, periodic, _ = CASES[name]
    return MultispinGlass3D(shape, TS, couplings=couplings_of(name), periodic=periodic, replicas=A, seed=SEED, route=route)


def swap_seeds():
    return [SWAP_SEED + s for s in range(S)]


def twin_run(name):
    """ROUNDS rounds of K sweeps on a plain handle, the swaps decided by the twin on the handle's integers and applied on the host.
    Computed once per case: the planes, each round's measurement, the book."""
    if name in _twin_run:
        return _twin_run[name]
    g = plain(name)
    book = twin.Book(A, S, len(TS))
    rows = []
    try:
        for _ in range(ROUNDS):
            g.sweep(K)
            unsat, ssum, q, ql = g._msc.measure()
            rows.append((unsat, ssum, q, ql))
            accept = twin.swap_pass(book, TS, 2 * unsat - g.n_bonds, swap_seeds())
            g._msc.set_planes(twin.exchange(g._msc.get_planes(), twin.pack_masks(accept)))
        out = {"planes": g._msc.get_planes(), "rows": [np.stack(c) for c in zip(*rows)], "book": book, "nb": g.n_bonds, "N": g.n_spins}
    finally:
        g.close()
    _twin_run[name] = out
    return out


def check_history(h, rows, nb, N):
    unsat, ssum, q, ql = rows
    assert h["E"].dtype == np.float64 and h["E"].shape == unsat.shape
    assert (h["E"] == 2 * unsat - nb).all() and (h["M"] == ssum / N).all()
    assert (h["q"] == q / N).all() and (h["q_link"] == ql / nb).all()


@pytest.mark.parametrize("route", ["small", "hbm"])
@pytest.mark.parametrize("name", list(CASES))
def test_without_swaps_it_is_the_plain_glass(name, route):
    """The no-regression anchor: run(n, k, swap=False) leaves the planes of sweep(n k), and the rows are measure() after each k."""
    pt, g = tempering(name, route), plain(name, route)
    try:
        assert pt.route == route
        h = pt.run(3, K, swap=False)
        rows = []
        for _ in range(3):
            g.sweep(K)
            rows.append(g._msc.measure())
        assert (pt._msc.get_planes() == g._msc.get_planes()).all()
        check_history(h, [np.stack(c) for c in zip(*rows)], g.n_bonds, g.n_spins)
        st = pt.stats()
        assert not st["attempts"].any() and not st["round_trips"].any()
        assert (st["label_at_slot"] == np.arange(len(TS))).all()
        assert pt.sweep_count == 3 * K and pt.round_count == 3 and pt.launch_count == g.launch_count
    finally:
        pt.close()
        g.close()


@pytest.mark.parametrize("route", ["small", "hbm"])
@pytest.mark.parametrize("name", list(CASES))
def test_with_swaps_it_is_the_twin(name, route):
    """Every word of every plane after 6 rounds, every row of the record and every counter equal the twin's, which is fed the plain
    handle's integers; the pad bits (never swapped) equal those of the run without swaps."""
    ref = twin_run(name)
    pt, g = tempering(name, route), plain(name, route)
    try:
        h = pt.run(ROUNDS, K)
        got = pt._msc.get_planes()
        assert (got == ref["planes"]).all(), f"{int((got != ref['planes']).sum())} words differ"
        check_history(h, ref["rows"], ref["nb"], ref["N"])
        st, book = pt.stats(), ref["book"]
        assert (st["attempts"] == book.attempts).all() and (st["accepts"] == book.accepts).all()
        assert (st["label_at_slot"] == book.labels).all() and (st["flags"] == book.flags).all()
        assert (st["round_trips"] == book.trips).all()
        assert (st["attempts"] == ROUNDS).all() and 0 < st["accepts"].sum() < st["attempts"].sum()
        assert (st["label_at_slot"] != np.arange(len(TS))).any()
        with np.errstate(invalid="ignore"):
            assert (pt.acceptance() == book.accepts.sum(axis=0) / book.attempts.sum(axis=0)).all()
        assert (pt.round_trips() == book.trips.sum(axis=(0, 2))).all()
        assert (pt.label_at_slot() == np.moveaxis(book.labels, 0, 1)).all()
        g.sweep(ROUNDS * K)
        keep = ~np.uint64((1 << (S % 64)) - 1)
        assert ((got[:, :, -1] & keep) == (g._msc.get_planes()[:, :, -1] & keep)).all()
    finally:
        pt.close()
        g.close()


def test_with_swaps_it_is_the_single_lattices():
    """Samples 0, 1, 63, 64, 69 of the cube rebuilt from IsingModel3D: one model per slot and replica with the slot's seed,
    gibbs_update(k), energy(), the twin's pass, the spins exchanged through the setter.  Ties the contract to K8's sweep."""
    from tsu.models import IsingModel3D
    name, pick = "cube", (0, 1, 63, 64, 69)
    shape, periodic, _ = CASES[name]
    j = couplings_of(name)
    nT = len(TS)
    models = [[[IsingModel3D(shape, temperature=T, periodic=periodic, seed=SEED + a * nT + t, couplings=tuple(x[s] for x in j))
                for s in pick] for a in range(A)] for t, T in enumerate(TS)]
    book = twin.Book(A, len(pick), nT)
    seeds = [SWAP_SEED + s for s in pick]
    pt = tempering(name, None)
    try:
        for _ in range(ROUNDS):
            E = np.zeros((nT, A, len(pick)))
            for t in range(nT):
                for a in range(A):
                    for k, m in enumerate(models[t][a]):
                        m.gibbs_update(K)
                        E[t, a, k] = m.energy()
            accept = twin.swap_pass(book, TS, E, seeds)
            spins = np.array([[[m.spins.reshape(shape) for m in models[t][a]] for a in range(A)] for t in range(nT)])
            moved = twin.exchange_unpacked(spins, accept)
            for t in range(nT):
                for a in range(A):
                    for k, m in enumerate(models[t][a]):
                        m.spins = moved[t, a, k]
        pt.run(ROUNDS, K)
        got = pt.spin_array()
        for t in range(nT):
            for a in range(A):
                for k, s in enumerate(pick):
                    assert (got[t, a, s] == models[t][a][k].spins.reshape(shape)).all(), (t, a, s)
        assert (pt.stats()["label_at_slot"][:, list(pick)] == book.labels).all()
        assert book.accepts.sum() > 0
    finally:
        pt.close()
        for row in models:
            for pair in row:
                for m in pair:
                    m._lat.close()


@pytest.mark.parametrize("route", ["small", "hbm"])
def test_forced_passes(route):
    """Rounds without sweeps (swap_interval = 0), so the energies are the ones set.  Per sample the slots are filled with five
    configurations of five distinct energies, sorted by the test.

    Energies strictly decreasing with slot while T increases: every delta > 0, every pair accepts, the slot-0 configuration arrives
    at the top in one pass and every other one moves down by one (the composition of consecutive exchanges the apply kernel
    streams).  This is the ordering under which 'every delta >= 0' holds: delta = (1/T_i - 1/T_{i+1}) (E_x - E_y) has a positive
    first factor, so it needs E_x > E_y.  Samples 64 w + b with b % 3 == 1 get the opposite ordering instead, which with T from 0.1
    to 50 and energy gaps of at least 4 makes an accept rare (the test asserts what the twin says, and that it is no accept at the
    coldest pair); b % 3 == 2 keep a random order.  So the masks of one word are neither 0 nor all ones."""
    from tsu.models import MultispinTempering3D
    shape, periodic, _ = CASES["cube"]
    Ts = (0.1, 0.5, 2.0, 10.0, 50.0)
    nT = len(Ts)
    j = couplings_of("cube")
    pt = MultispinTempering3D(shape, Ts, couplings=j, periodic=periodic, replicas=A, seed=SEED, swap_seed=SWAP_SEED, route=route,
                              initial="up")
    try:
        # candidate configurations per sample: all up with the first n sites of a random order flipped, n < N / 2
        rng = np.random.default_rng(12)
        N = pt.n_spins
        order = np.stack([rng.permutation(N) for _ in range(S)])
        cand = np.ones((N // 2, S, N), np.int8)
        for n in range(N // 2):
            for s in range(S):
                cand[n, s, order[s, :n]] = -1
        E = np.stack([msc.reference_energy(cand[n].reshape((S,) + shape), periodic, j) for n in range(N // 2)])  # (N / 2, S)
        spins = np.zeros((nT, A, S, N), np.int8)
        for s in range(S):
            levels = np.unique(E[:, s])
            assert levels.size >= nT, "fewer than five distinct energies among the candidates"
            chosen = [int(np.flatnonzero(E[:, s] == e)[0]) for e in levels[:nT]]  # ascending energy
            if s % 64 % 3 == 0:
                chosen = chosen[::-1]  # descending with slot: every pair accepts
            elif s % 64 % 3 == 2:
                chosen = list(rng.permutation(chosen))
            for t in range(nT):
                spins[t, :, s] = cand[chosen[t], s]
        planes = np.stack([np.stack([msc.pack(spins[t, a].reshape((S,) + shape) == 1) for a in range(A)]) for t in range(nT)])
        pt._msc.set_planes(planes)
        h = pt.run(1, 0)
        book = twin.Book(A, S, nT)
        accept = twin.swap_pass(book, Ts, h["E"][0], [SWAP_SEED + s for s in range(S)])
        up, down = [s for s in range(S) if s % 64 % 3 == 0], [s for s in range(S) if s % 64 % 3 == 1]
        assert accept[:, :, up].all() and not accept[0][:, down].any()
        masks = twin.pack_masks(accept)
        assert ((masks != 0) & (masks != np.uint64(0xFFFFFFFFFFFFFFFF))).all()
        got = pt._msc.get_planes()
        assert (got == twin.exchange(planes, masks)).all()
        after = pt.spin_array().reshape(nT, A, S, N)
        for s in up:
            assert (after[nT - 1, :, s] == spins[0, :, s]).all() and (after[:nT - 1, :, s] == spins[1:, :, s]).all()
        st = pt.stats()
        assert (st["accepts"] == book.accepts).all() and (st["label_at_slot"] == book.labels).all()
        assert (st["flags"] == book.flags).all() and (st["label_at_slot"][:, up] == np.r_[1:nT, 0]).all()
        assert (st["flags"][:, up, 0] == twin.TOP).all() and (st["flags"][:, up, 1] == twin.BOTTOM).all()
        # the same arrangement set again before each further pass: the labels rotate, and after n_temps passes label 0, TOP since the
        # first, is back at slot 0 of the forced samples: exactly one round trip
        for _ in range(nT - 1):
            pt._msc.set_planes(planes)
            h = pt.run(1, 0)
            twin.swap_pass(book, Ts, h["E"][0], [SWAP_SEED + s for s in range(S)])
        st = pt.stats()
        assert (st["label_at_slot"] == book.labels).all() and (st["round_trips"] == book.trips).all()
        assert (st["flags"] == book.flags).all() and (st["accepts"] == book.accepts).all()
        assert (st["label_at_slot"][:, up] == np.arange(nT)).all()
        assert (st["round_trips"][:, up, 0] == 1).all() and not st["round_trips"][:, up, 1:].any()
        assert pt.sweep_count == 0 and pt.round_count == nT
    finally:
        pt.close()


def test_a_ladder_of_256_temperatures():
    """4 x 4 x 4, S = 64, 256 slots: the plan kernel's per-lane tables at their limit, two rounds against the twin."""
    from tsu.models import MultispinGlass3D, MultispinTempering3D, edwards_anderson_samples
    shape, n, Ts = (4, 4, 4), 64, np.linspace(0.4, 3.0, 256)
    j = edwards_anderson_samples(shape, n, kind="bimodal", seed=3)
    seeds = [SWAP_SEED + s for s in range(n)]
    pt = MultispinTempering3D(shape, Ts, couplings=j, seed=SEED, swap_seed=SWAP_SEED)
    g = MultispinGlass3D(shape, Ts, couplings=j, seed=SEED)
    book = twin.Book(1, n, 256)
    try:
        h = pt.run(2, 1)
        for r in range(2):
            g.sweep(1)
            unsat = g._msc.measure()[0]
            assert (h["E"][r] == 2 * unsat[:, 0] - g.n_bonds).all()
            accept = twin.swap_pass(book, Ts, 2 * unsat - g.n_bonds, seeds)
            g._msc.set_planes(twin.exchange(g._msc.get_planes(), twin.pack_masks(accept)))
        assert (pt._msc.get_planes() == g._msc.get_planes()).all()
        st = pt.stats()
        assert (st["accepts"] == book.accepts).all() and (st["label_at_slot"] == book.labels).all()
        assert (st["flags"] == book.flags).all() and (st["round_trips"] == book.trips).all()
        assert st["accepts"].sum() > 1000 and (np.abs(st["label_at_slot"] - np.arange(256)) >= 2).any()
    finally:
        pt.close()
        g.close()


# ---------------------------------------------------------------- equilibrium against exact enumeration
ENUM = dict(shape=(2, 3, 2), periodic=False, S=8, Ts=(0.5, 1.0, 1.5, 2.0), dseed=21, seed=5, swap_seed=77, discard=400, batches=20,
            per_batch=200)


def enum_couplings():
    from tsu.models import edwards_anderson_samples
    return edwards_anderson_samples(ENUM["shape"], ENUM["S"], kind="bimodal", seed=ENUM["dseed"], periodic=ENUM["periodic"])


def exact_enumeration(shape, jr, jd, jl, Ts):
    """(<E>, <q^2>) per temperature of one open-boundary sample by enumerating every state; q of two independent replicas."""
    D, R, C = shape
    N = D * R * C
    idx = np.arange(2 ** N, dtype=np.int64)
    st = np.stack([1 - 2 * ((idx >> n) & 1) for n in range(N)], axis=1).astype(np.float64)
    site = lambda z, r, c: (z * R + r) * C + c  # noqa: E731
    E = np.zeros(2 ** N)
    for z in range(D):
        for r in range(R):
            for c in range(C):
                n = site(z, r, c)
                if c + 1 < C:
                    E -= float(jr[z, r, c]) * st[:, n] * st[:, site(z, r, c + 1)]
                if r + 1 < R:
                    E -= float(jd[z, r, c]) * st[:, n] * st[:, site(z, r + 1, c)]
                if z + 1 < D:
                    E -= float(jl[z, r, c]) * st[:, n] * st[:, site(z + 1, r, c)]
    out = []
    for T in Ts:
        w = np.exp(-(E - E.min()) / T)
        w /= w.sum()
        Cm = st.T @ (st * w[:, None])
        out.append((float(w @ E), float((Cm ** 2).sum()) / N ** 2))
    return out


def enum_deviations(E, q, exact_of_sample):
    """E (n, nT, S) of replica 0, q (n, nT, S) as q / N: rows (sample, slot, observable, mean, exact, standard error) from
    ENUM['batches'] batch means."""
    nb = ENUM["batches"]
    rows = []
    for s, exact in enumerate(exact_of_sample):
        for t, (e_ex, q2_ex) in enumerate(exact):
            for name, x, ex in (("E", E[:, t, s], e_ex), ("q2", q[:, t, s] ** 2, q2_ex)):
                b = x.reshape(nb, -1).mean(axis=1)
                rows.append((s, t, name, float(b.mean()), ex, float(b.std(ddof=1) / math.sqrt(nb))))
    return rows


def test_equilibrium_against_exact_enumeration():
    """An open 2 x 3 x 2 glass (12 sites, 4096 states), 8 samples, 4 temperatures 0.5 .. 2.0, two replicas, a swap pass after every
    sweep: 400 discarded rounds, 4000 recorded ones in 20 batches; <E> and <q^2> per sample and slot within 4 batch-means standard
    errors of the enumeration.  An inverted acceptance ratio fails here (the twin comparison would not notice: the twin would share
    it).

    Seeds and lengths were fixed by rehearsing this very run on the CPU (multispin_pt_twin.Tempering: the bit-sliced sweep plus the
    twin's pass) before the device saw it; the first pair tried (seed 5, swap seed 77) met the rule and was kept.  Worst deviation
    of the rehearsal over its 64 figures: 2.96 standard errors (<q^2> of sample 7 at T = 1.5), next 2.46 and 2.28; acceptance per
    sample and pair 0.50 ... 0.76; 2272 ... 3160 round trips per sample.  The same rehearsal with the ratio inverted
    (E_y - E_x) misses by up to 79 standard errors.  The first device run gave the rehearsal's figures digit for digit: worst
    2.96.  A device run that disagrees is a finding, not a reason to pick other seeds.
    """
    from tsu.models import MultispinTempering3D
    j = enum_couplings()
    pt = MultispinTempering3D(ENUM["shape"], ENUM["Ts"], couplings=j, periodic=ENUM["periodic"], replicas=2, seed=ENUM["seed"],
                              swap_seed=ENUM["swap_seed"], initial="up")
    try:
        pt.run(ENUM["discard"], 1, record=False)
        Es, qs = [], []
        for _ in range(ENUM["batches"]):
            h = pt.run(ENUM["per_batch"], 1)
            Es.append(h["E"][:, :, 0])
            qs.append(h["q"])
        exact = [exact_enumeration(ENUM["shape"], j[0][s], j[1][s], j[2][s], ENUM["Ts"]) for s in range(ENUM["S"])]
        worst = 0.0
        for s, t, name, mean, ex, se in enum_deviations(np.concatenate(Es), np.concatenate(qs), exact):
            dev = abs(mean - ex) / se
            print(f"sample {s} T={ENUM['Ts'][t]} {name}: mean={mean:.5f} exact={ex:.5f} se={se:.2e} dev={dev:.2f}")
            worst = max(worst, dev)
            assert abs(mean - ex) < 4 * se, (s, t, name, mean, ex, se)
        acc = pt.acceptance()
        print(f"worst deviation {worst:.2f} se; acceptance {acc.min():.3f} .. {acc.max():.3f}; round trips {pt.round_trips()}")
        assert (acc > 0).all() and (pt.round_trips() >= 1).all()
    finally:
        pt.close()


@pytest.mark.parametrize("route,per_round", [("small", 1), ("hbm", 2 * K)])
def test_launch_counts_and_continuation(route, per_round):
    """A round is the sweep launches of the plain glass plus one measurement, one plan and one exchange; run(3) then run(2) is
    run(5): the sweep and round counters, the counters of the passes and the stream of swap uniforms continue."""
    a, b = tempering("cube", route), tempering("cube", route)
    try:
        assert a.launch_count == 0 and a.swap_launch_count == 0
        a.run(3, K, record=False)
        assert a.launch_count == 3 * per_round and a.swap_launch_count == 3 * 3
        h = a.run(2, K)
        assert a.launch_count == 5 * per_round and a.swap_launch_count == 5 * 3
        assert h["E"].shape == (2, len(TS), A, S) and a.round_count == 5 and a.sweep_count == 5 * K
        a.run(1, K, swap=False, record=True)
        assert a.swap_launch_count == 5 * 3 + 1
        a.run(1, K, swap=False, record=False)
        assert a.swap_launch_count == 5 * 3 + 1 and a.launch_count == 7 * per_round
        hb = b.run(5, K)
        b.run(2, K, swap=False, record=False)
        assert (hb["E"][3:] == h["E"]).all() and (hb["q_link"][3:] == h["q_link"]).all()
        assert (a._msc.get_planes() == b._msc.get_planes()).all()
        sa, sb = a.stats(), b.stats()
        assert all((sa[k] == sb[k]).all() for k in sa) and (sa["attempts"] == 5).all()
    finally:
        a.close()
        b.close()


def test_the_scan_returns_the_documented_keys():
    from tsu.models import edwards_anderson_samples, multispin_tempering_scan_3d
    shape, n, Ts = (4, 4, 4), 64, [0.8, 1.2, 1.8, 3.0]
    j = edwards_anderson_samples(shape, n, kind="bimodal", seed=8)
    res = multispin_tempering_scan_3d(shape, Ts, couplings=j, n_equilibrate=40, n_measure=20, measure_every=4, swap_interval=2, seed=1)
    for k in ("energy", "magnetization", "overlap", "overlap_sq", "overlap_4", "link_overlap"):
        assert res[k].shape == (n, len(Ts)), k
    assert res["acceptance"].shape == (n, len(Ts) - 1) and res["round_trips"].shape == (n,)
    # 120 attempts per sample and pair: a single entry may well be 0, a pair's mean over the samples may not
    assert ((res["acceptance"] >= 0) & (res["acceptance"] <= 1)).all() and (res["acceptance"].mean(axis=0) > 0).all()
    assert (res["temperatures"] == np.asarray(Ts)).all()
    avg = res["average"]
    for k in ("energy", "magnetization", "overlap", "overlap_sq", "link_overlap"):
        assert avg[k].shape == (len(Ts),) and np.isfinite(avg[k]).all() and avg[k + "_err"].shape == (len(Ts),), k
    assert avg["binder"].shape == (len(Ts),) and (np.diff(avg["energy"]) > 0).all()
    assert ((res["overlap_sq"] >= 0) & (res["overlap_sq"] <= 1)).all() and (np.abs(res["link_overlap"]) <= 1).all()

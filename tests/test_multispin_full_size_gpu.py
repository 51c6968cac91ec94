"""K9 on the GPU where its grids split, at its limits and far ends: every word of get_planes() and every integer of measure(), of the
record and of the swap counters against the NumPy twins (tests/helpers/multispin_shapes.py holds the cases and the twins' runs, and
tests/test_multispin_full_size_cpu.py what those runs must contain).  Nothing here has a tolerance.

  1  sweeps and measure() at 2048 octets (8 k9_sweep workgroups per plane), rows of 65 octets, a last workgroup with dead waves,
     two k9_measure workgroups on one output column, both bounds of k9_small at once, 65280 planes
  2  k9_measure with every lane's counters at 192, the design maximum, against closed forms
  3  ladders of 2, 9, 10, 17, 18 and 33 slots: the look-ahead of k9_pt_apply and the chunks of k9_pt_plan, with pad lanes, a second
     word and replica 1's tag; swaps on a 32^3 plane
  4  the scratch ring of run(record=False) over three laps, and the record buffer shrinking and growing
  5  seeds with the top bit set, swap seeds that carry into the high key word, the sweep counter up to hs = 2^32 - 1, the round
     counter up to 2^32 - 1, and the refusals beyond
"""
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


shapes = _load("multispin_shapes")
pt_twin, msc, fe = shapes.pt_twin, shapes.msc, shapes.fe


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert (got == want).all(), f"{what}: {int((got != want).sum())} of {got.size} differ, first at {np.argwhere(got != want)[:3].tolist()}"


def check_history(h, rows, nb, N):
    unsat, ssum, q, ql = rows
    assert h["E"].dtype == np.float64
    same(h["E"], (2 * unsat - nb).astype(np.float64), "E of the record")
    same(h["M"], ssum / N, "M of the record")
    same(h["q"], q / N, "q of the record")
    same(h["q_link"], ql / nb, "q_link of the record")


def check_state(pt, run, stop):
    """Planes and every counter of the handle against the twin's snapshot after `stop` rounds."""
    planes, book = run.snap[stop]
    same(pt._msc.get_planes(), planes, f"planes after {stop} rounds")
    st = pt.stats()
    same(st["attempts"], book.attempts, "attempts")
    same(st["accepts"], book.accepts, "accepts")
    same(st["label_at_slot"], book.labels, "labels")
    same(st["flags"], book.flags, "flags")
    same(st["round_trips"], book.trips, "round trips")


def tempering(run, route, **kw):
    from tsu.models import MultispinTempering3D
    j, _ = shapes.couplings(run.shape, run.periodic, run.S)
    pt = MultispinTempering3D(run.shape, run.Ts, couplings=j, periodic=run.periodic, replicas=run.A, seeds=run.seeds,
                              swap_seed=fe.SEED_CARRY, route=route, **kw)
    assert pt.swap_seeds == run.swap_seeds
    return pt


# ------------------------------------------------------------------------------------------------------------ 1. sweeps
def single_lattices(g, c, ref, got, unsat):
    """Samples 0, 63, 64 and S - 1 of slot 0, both replicas, rebuilt with IsingModel3D on the sample's couplings and the plane's seed:
    ties the large shapes to K8's sweep, not only to the bit-sliced twin."""
    from tsu.models import IsingModel3D
    j, _ = shapes.couplings(c["shape"], c["periodic"], c["S"])
    for a in range(c["A"]):
        for s in shapes.PICK(c["S"]):
            m = IsingModel3D(c["shape"], temperature=c["Ts"][0], periodic=c["periodic"], seed=ref["seeds"][0][a],
                             couplings=tuple(x[s] for x in j))
            try:
                m.sweep_count = c["sweep0"]
                for n in c["calls"]:
                    m.gibbs_update(n)
                bit = (got[0, a, s // 64] >> np.uint64(s % 64)) & np.uint64(1)
                same(np.where(bit == 1, 1, -1).astype(np.int8), m.spins.reshape(c["shape"]), f"sample {s} of replica {a}")
                assert 2 * unsat[0, a, s] - ref["nb"] == m.energy() and g.energies()[0, a, s] == m.energy()
            finally:
                m._lat.close()


@pytest.mark.parametrize("name,route", [(n, r) for n, c in shapes.SWEEPS.items() for r in c["routes"]])
def test_sweeps_and_measurement_are_the_twin(name, route):
    from tsu.models import MultispinGlass3D
    c, ref = shapes.SWEEPS[name], shapes.sweep_case(name)
    j, _ = shapes.couplings(c["shape"], c["periodic"], c["S"])
    g = MultispinGlass3D(c["shape"], c["Ts"], couplings=j, periodic=c["periodic"], replicas=c["A"], seeds=ref["seeds"], route=route)
    try:
        assert g.route == (route or "small") and g.n_bonds == ref["nb"]
        same(g._msc.get_planes(), ref["start"], "the start (k9_randomize)")
        g.sweep_count = c["sweep0"]
        for n in c["calls"]:
            g.sweep(n)
        assert g.sweep_count == c["sweep0"] + sum(c["calls"])
        assert g.launch_count == (len(c["calls"]) if g.route == "small" else 2 * sum(c["calls"]))
        got = g._msc.get_planes()
        same(got, ref["planes"], "planes")
        unsat, ssum, q, ql = g._msc.measure()
        same(unsat, ref["unsat"], "unsat")
        same(ssum, ref["sum"], "sum")
        if c["A"] == 2:
            same(q, ref["q"], "q")
            same(ql, ref["ql"], "q_link")
        else:
            assert q is None and ql is None
        if name in ("cube32", "small_limit"):
            single_lattices(g, c, ref, got, unsat)
    finally:
        g.close()


def test_the_small_route_ends_at_its_bounds():
    """One step past either bound of msc_fits_small: auto takes the HBM route, route='small' is refused."""
    from tsu import _hip
    from tsu.models import MultispinGlass3D, edwards_anderson_samples
    for shape, _ in shapes.TOO_LARGE_FOR_SMALL:
        j = edwards_anderson_samples(shape, 1, kind="bimodal", seed=5)
        with pytest.raises(_hip.UnsupportedError, match="small route"):
            MultispinGlass3D(shape, [1.0], couplings=j, seed=1, route="small")
        g = MultispinGlass3D(shape, [1.0], couplings=j, seed=1)
        assert g.route == "hbm"
        g.close()


# ------------------------------------------------------------------------------------------------------------ 2. measurement
@pytest.mark.parametrize("name", list(shapes.MEASURE))
def test_measure_at_the_top_of_its_counters(name):
    """Constructed planes (multispin_shapes.measure_case): samples whose every bond is unsatisfied, or differs between the replicas,
    take every lane's 8-plane counter to 3 x 64 = 192.  Closed forms and the twin, through measure() and through a recorded row.
    A tempering handle needs two slots: slot 1 holds slot 0's planes with the replicas exchanged."""
    from tsu.models import MultispinTempering3D
    shape, per = shapes.MEASURE[name]
    m = shapes.measure_case(name)
    planes = np.concatenate([m["planes"], m["planes"][:, ::-1]])
    want = pt_twin.measure(planes, per, *m["packed"], 64)
    pt = MultispinTempering3D(shape, [1.0, 2.0], couplings=m["j"], periodic=per, replicas=2, seed=fe.SEED_HI, swap_seed=1, initial="up")
    try:
        assert pt.route == "hbm" and pt.n_bonds == m["nb"] == want[4]
        pt._msc.set_planes(planes)
        direct = pt._msc.measure()
        pt.run(1, 0, swap=False)
        row = tuple(x[0] for x in pt._msc.pt_history(1))
        same(pt._msc.get_planes(), planes, "planes after a round without sweeps or swaps")
        for got in (direct, row):
            for k, what in enumerate(("unsat", "sum", "q", "q_link")):
                same(got[k], want[k], what)
            unsat, ssum, q, ql = got
            for b in range(64):
                closed = m["closed"].get(b % 4)
                if closed is None:
                    continue
                for t in (0, 1):  # slot 1: the replicas exchanged
                    assert tuple(unsat[t, ::1 - 2 * t, b]) == closed["unsat"] and tuple(ssum[t, ::1 - 2 * t, b]) == closed["sum"], (t, b)
                    assert q[t, b] == closed["q"] and ql[t, b] == closed["ql"], (t, b)
        if name == "cube32":
            assert direct[0][0, 0, 0] == 98304 and direct[3][0, 1] == -98304
    finally:
        pt.close()


# ------------------------------------------------------------------------------------------------------------ 3. ladders
@pytest.mark.parametrize("n_temps,route", [(n, r) for n, routes in shapes.LADDERS.items() for r in routes])
def test_ladders_at_the_chunk_edges(n_temps, route):
    run = shapes.ladder_run(n_temps)
    acc = run.twin.book.accepts.sum()
    assert 0 < acc < run.twin.book.attempts.sum() and (n_temps < 9 or run.mixed_mask_words() > 0)
    pt = tempering(run, route)
    try:
        assert pt.route == (route or "small")
        same(pt._msc.get_planes(), run.start, "the start")
        h = pt.run(shapes.LADDER_ROUNDS, shapes.LADDER_K)
        check_state(pt, run, shapes.LADDER_ROUNDS)
        check_history(h, run.rows_of(0, shapes.LADDER_ROUNDS), pt.n_bonds, pt.n_spins)
        assert pt.round_count == shapes.LADDER_ROUNDS and pt.sweep_count == shapes.LADDER_ROUNDS * shapes.LADDER_K
    finally:
        pt.close()


def test_swaps_on_a_plane_of_many_workgroups():
    """32^3, temperatures (1.50, 1.51, 1.52): k9_pt_apply over 128 workgroups per (replica, word), k9_measure over two."""
    run = shapes.cube32_ladder_run()
    book = run.twin.book
    acc, att = book.accepts.sum(axis=(0, 1)), book.attempts.sum(axis=(0, 1))
    assert ((0 < acc) & (acc < att)).all(), (acc, att)
    pt = tempering(run, "hbm")
    try:
        same(pt._msc.get_planes(), run.start, "the start")
        h = pt.run(shapes.CUBE32_ROUNDS, shapes.CUBE32_K)
        check_state(pt, run, shapes.CUBE32_ROUNDS)
        check_history(h, run.rows_of(0, shapes.CUBE32_ROUNDS), pt.n_bonds, pt.n_spins)
    finally:
        pt.close()


# ------------------------------------------------------------------------------------------------------------ 4. the ring
@pytest.mark.parametrize("route", ["small", "hbm"])
@pytest.mark.parametrize("unrecorded", [130, 65])
def test_the_scratch_ring_over_its_laps(unrecorded, route):
    """run(n, 1, record=False) then run(1, 1): n = 130 is two full laps of the 64-row ring and a lap of 2, n = 65 one lap and a lap
    of 1.  A row left unzeroed on a later lap would corrupt the energies, and through them the swaps, of every later round."""
    run = shapes.ring_run()
    pt = tempering(run, route)
    try:
        assert pt.run(unrecorded, 1, record=False) is None
        h = pt.run(1, 1)
        check_state(pt, run, unrecorded + 1)
        check_history(h, run.rows_of(unrecorded, 1), pt.n_bonds, pt.n_spins)
        assert pt.round_count == pt.sweep_count == unrecorded + 1
    finally:
        pt.close()


@pytest.mark.parametrize("route", ["small", "hbm"])
def test_the_record_shrinks_and_grows(route):
    """On one handle: 5 recorded rounds, 2 (shorter than the buffer held), 70 without a record (the ring takes the buffer over), 9."""
    run = shapes.ring_run()
    pt = tempering(run, route)
    try:
        done = 0
        for n, record in ((5, True), (2, True), (70, False), (9, True)):
            h = pt.run(n, 1, record=record)
            check_state(pt, run, done + n)
            if record:
                assert h["E"].shape[0] == n
                check_history(h, run.rows_of(done, n), pt.n_bonds, pt.n_spins)
                for wrong in (n - 1, n + 1):
                    with pytest.raises(ValueError, match=f"recorded {n} rounds"):
                        pt._msc.pt_history(wrong)
            else:
                assert h is None and pt._msc.pt_history(0)[0].shape[0] == 0
                with pytest.raises(ValueError, match="recorded 0 rounds"):
                    pt._msc.pt_history(n)
            done += n
        assert done == shapes.RING_STOPS[-2]
    finally:
        pt.close()


# ------------------------------------------------------------------------------------------------------------ 5. far ends
@pytest.mark.parametrize("route", ["small", "hbm"])
@pytest.mark.parametrize("name", list(shapes.PT_CASES))
def test_far_ends_of_the_counters_and_seeds(name, route):
    """Seeds SEED_HI + index, swap seeds SEED_CARRY + s.  `straddle`: the half-sweep counter crosses 2^31 and the round counter 2^31;
    `end`: the last half-sweep is hs = 2^32 - 1 and the last round 2^32 - 1.  Beyond, run() refuses and changes nothing."""
    from tsu import _hip
    for position in ("straddle", "end"):
        run = shapes.far_run(name, position)
        assert 0 < run.twin.book.accepts.sum() < run.twin.book.attempts.sum()
        pt = tempering(run, route)
        try:
            pt.sweep_count, pt.round_count = shapes.FAR_POSITIONS[position]
            h = pt.run(shapes.FAR_ROUNDS, shapes.FAR_K)
            check_state(pt, run, shapes.FAR_ROUNDS)
            check_history(h, run.rows_of(0, shapes.FAR_ROUNDS), pt.n_bonds, pt.n_spins)
            if position != "end":
                continue
            assert pt.sweep_count == 2 ** 31 and pt.round_count == 2 ** 32
            launches = (pt.launch_count, pt.swap_launch_count)
            with pytest.raises(ValueError, match="sweep counter overflow"):
                pt.run(1, 1)
            with pytest.raises(ValueError, match="round counter overflow"):
                pt.run(1, 0)
            # the library's own checks, below the wrapper's
            ctx, lib = pt._msc.ctx, pt._msc.lib
            for args, text in (((1, 1, 1, 1, 2 ** 31, 0), "sweep counter overflow"), ((3, 2, 1, 1, 2 ** 31 - 5, 0), "sweep counter overflow"),
                               ((2, 0, 1, 1, 0, 2 ** 32 - 1), "round counter overflow")):
                assert lib.tsu_msc_pt_run(pt._msc.h, *args) == _hip.TSU_E_INVALID
                assert text in lib.tsu_last_error(ctx.h).decode()
            assert pt.sweep_count == 2 ** 31 and pt.round_count == 2 ** 32 and launches == (pt.launch_count, pt.swap_launch_count)
            check_state(pt, run, shapes.FAR_ROUNDS)
            check_history(pt.history(), run.rows_of(0, shapes.FAR_ROUNDS), pt.n_bonds, pt.n_spins)
        finally:
            pt.close()


@pytest.mark.parametrize("route", ["small", "hbm"])
def test_the_plain_glass_stops_at_its_last_sweep(route):
    """sweep(1) from 2^31 - 1 is hs = 2^32 - 2 and 2^32 - 1 and equals the twin; one more is refused and changes nothing."""
    from tsu.models import MultispinGlass3D
    shape, per = shapes.PT_CASES["cube"]
    S, Ts = shapes.PT_S, shapes.PT_TS[:2]
    j, packed = shapes.couplings(shape, per, S)
    seeds = shapes.plane_seeds(len(Ts), 1)
    g = MultispinGlass3D(shape, Ts, couplings=j, periodic=per, seeds=seeds, route=route)
    try:
        start = g._msc.get_planes()
        g.sweep_count = fe.end(1)
        g.sweep(1)
        want = np.stack([msc.bitsliced_sweep(start[t, 0], per, *packed, T, 1, seeds[t][0], fe.end(1))[None] for t, T in enumerate(Ts)])
        same(g._msc.get_planes(), want, "planes after the last sweep")
        assert (want != np.stack([msc.bitsliced_sweep(start[t, 0], per, *packed, T, 1, seeds[t][0], 0)[None] for t, T in enumerate(Ts)])).any()
        launches = g.launch_count
        with pytest.raises(ValueError, match="sweep counter overflow"):
            g.sweep(1)
        assert g.sweep_count == 2 ** 31 and g.launch_count == launches
        same(g._msc.get_planes(), want, "planes after the refused sweep")
    finally:
        g.close()

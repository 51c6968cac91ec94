"""The inputs of tests/test_multispin_full_size_gpu.py, checked on the host (no GPU needed): at the shapes that split K9's grids the
bit-sliced twin is the per-sample twin, its integers are the per-sample energies, and the runs hold what the device comparison
needs: a hi16 tie, swaps accepted and refused, mask words that are neither 0 nor all ones, and far-end results that differ from those
at counter 0 (so a kernel that dropped the top bits of a counter or a seed could not pass)."""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


shapes = _load("multispin_shapes")
pt_twin, msc, fe = shapes.pt_twin, shapes.msc, shapes.fe


def test_the_table_reaches_what_it_says():
    """The arithmetic of the case table against the kernels' constants: 256 octets per k9_sweep workgroup, 16384 sites per k9_measure
    workgroup, 8192 sites and 1024 octets on the small route, 65535 planes."""
    geo = {}
    for name, c in shapes.SWEEPS.items():
        D, R, C = c["shape"]
        noct = (C + 15) // 16
        planes = len(c["Ts"]) * c["A"] * ((c["S"] + 63) // 64)
        geo[name] = (D * R * C, D * R * noct, noct, planes)
        assert planes <= 65535 and sum(c["calls"]) in (2, 5)
    assert geo["cube32"][:2] == (32768, 2048) and geo["cube32"][1] // 256 == 8 and geo["cube32"][0] == 2 * 16384
    assert geo["long_rows"] == (16480, 1040, 65, 2) and 1030 - 64 * 16 == 6 and 1040 - 4 * 256 == 16 and 16480 - 16384 == 96
    assert geo["odd_open"][:2] == (18414, 2046)
    assert geo["small_limit"][:2] == (8192, 1024) and geo["small_wide"][:3] == (8192, 512, 8)
    assert geo["many_planes"][3] == 65280 and 255 * 128 == 32640
    assert [(D * R * C, D * R * ((C + 15) // 16)) for (D, R, C), _ in shapes.TOO_LARGE_FOR_SMALL] == [(10240, 1024), (4608, 1152)]
    assert sum(c["sweep0"] != 0 for c in shapes.SWEEPS.values()) == 1
    far = shapes.SWEEPS["small_limit"]
    assert 2 * (far["sweep0"] + sum(far["calls"])) - 1 == 2 ** 32 - 1
    assert sorted(n - 1 for n in shapes.LADDERS) == [1, 8, 9, 16, 17, 32]
    assert shapes.swap_seeds(70)[1] >> 32 == 0 and shapes.swap_seeds(70)[2] >> 32 == 1
    assert all(s >> 63 for row in shapes.plane_seeds(5, 2) for s in row)
    (s0, r0), (s1, r1) = shapes.FAR_POSITIONS["straddle"], shapes.FAR_POSITIONS["end"]
    n = shapes.FAR_ROUNDS * shapes.FAR_K
    assert 2 * s0 < 2 ** 31 < 2 * (s0 + n) and r0 < 2 ** 31 < r0 + shapes.FAR_ROUNDS
    assert 2 * (s1 + n) - 1 == 2 ** 32 - 1 and r1 + shapes.FAR_ROUNDS - 1 == 2 ** 32 - 1


@pytest.mark.parametrize("name", ["cube32", "long_rows"])
def test_bitsliced_is_the_per_sample_twin_at_full_size(name):
    """Samples 0, 63, 64 and S - 1 through lattice3d_twin.sweep, from sweep0 = far_end.end(3) under SEED_HI; the twin's integers
    against the per-sample energies."""
    c = shapes.SWEEPS[name]
    shape, per, S, T = c["shape"], c["periodic"], c["S"], c["Ts"][0]
    j, packed = shapes.couplings(shape, per, S)
    pick = list(shapes.PICK(S))
    start = shapes.start_planes(shape, [[fe.SEED_HI]], (S + 63) // 64)[0, 0]
    # k9_randomize gives every sample of a plane the same start: make the samples differ before the sweep
    start ^= np.random.default_rng(5).integers(0, 2 ** 63, size=start.shape, dtype=np.uint64) << np.uint64(1)
    got = msc.bitsliced_sweep(start, per, *packed, T, 3, fe.SEED_HI, fe.end(3))
    spins = np.where(msc.unpack(start, S)[pick], 1, -1).astype(np.int8)
    jp = tuple(a[pick] for a in j)
    want = msc.reference_sweep(spins, per, jp, T, 3, fe.SEED_HI, fe.end(3))
    bits = msc.unpack(got, S)[pick]
    assert (np.where(bits, 1, -1) == want).all()
    assert (bits != msc.unpack(start, S)[pick]).any()
    unsat, ssum, q, ql, nb = pt_twin.measure(got[None, None], per, *packed, S)
    assert q is None and ql is None
    assert (2 * unsat[0, 0, pick] - nb == msc.reference_energy(want, per, jp)).all()
    assert (ssum[0, 0, pick] == want.reshape(len(pick), -1).sum(axis=1)).all()


def test_cube32_holds_a_tie_on_the_top_half():
    r = shapes.sweep_case("cube32")
    print("hi16 ties in the cube32 run:", r["ties"])
    assert r["ties"] >= 1
    assert (r["planes"] != r["start"]).any() and len(np.unique(r["planes"])) > 1000


def test_the_far_end_sweeps_differ_from_those_at_counter_zero():
    far, zero = shapes.sweep_case("small_limit"), shapes.sweep_case("small_limit", 0)
    assert (far["start"] == zero["start"]).all()
    assert (far["planes"] != zero["planes"]).any() and (far["unsat"] != zero["unsat"]).any()


def test_the_constructed_measurements_have_their_closed_forms():
    """The twin's integers on the constructed planes: the closed forms of samples b % 4 = 0, 1, 2, and on b % 4 = 3 the per-sample
    energy.  N_b drops the bonds the open axis lacks."""
    for name in shapes.MEASURE:
        shape, per = shapes.MEASURE[name]
        m = shapes.measure_case(name)
        assert m["nb"] == (3 * m["N"] if name == "cube32" else 3 * m["N"] - m["N"] // shape[1])
        unsat, ssum, q, ql, nb = pt_twin.measure(m["planes"], per, *m["packed"], 64)
        assert nb == m["nb"]
        for b in range(64):
            want = m["closed"].get(b % 4)
            if want is None:
                continue
            assert tuple(unsat[0, :, b]) == want["unsat"] and tuple(ssum[0, :, b]) == want["sum"], (name, b)
            assert q[0, b] == want["q"] and ql[0, b] == want["ql"], (name, b)
        pick = [3, 63]
        for a in range(2):
            spins = np.where(msc.unpack(m["planes"][0, a], 64)[pick], 1, -1).astype(np.int8)
            E = msc.reference_energy(spins, per, tuple(x[pick] for x in m["j"]))
            assert (2 * unsat[0, a, pick] - nb == E).all()
        assert len({int(x) for x in unsat[0, 0, 3::4]}) > 8


@pytest.mark.parametrize("n_temps", list(shapes.LADDERS))
def test_ladders_accept_and_refuse(n_temps):
    """Per ladder length: the accepts summed over samples are neither 0 nor all attempts; from 9 slots on some pass has a mask word
    that is neither 0 nor all ones."""
    r = shapes.ladder_run(n_temps)
    book = r.twin.book
    acc, att = book.accepts.sum(axis=(0, 1)), book.attempts.sum(axis=(0, 1))
    print(f"n_temps={n_temps}: accepts per pair {acc.tolist()} of {int(att[0])}; mixed mask words {r.mixed_mask_words()}")
    assert (att == shapes.LADDER_ROUNDS * shapes.LADDER_A * shapes.LADDER_S).all()
    assert 0 < acc.sum() < att.sum()
    if n_temps >= 9:
        assert r.mixed_mask_words() > 0
    assert book.rounds == shapes.LADDER_ROUNDS and r.twin.sweeps == shapes.LADDER_ROUNDS * shapes.LADDER_K


def test_the_cube32_ladder_accepts_and_refuses_at_every_pair():
    r = shapes.cube32_ladder_run()
    acc, att = r.twin.book.accepts.sum(axis=(0, 1)), r.twin.book.attempts.sum(axis=(0, 1))
    print("cube32 ladder: accepts per pair", acc.tolist(), "of", att.tolist())
    assert (att == shapes.CUBE32_ROUNDS * 2 * 70).all() and ((0 < acc) & (acc < att)).all()


@pytest.mark.parametrize("name", list(shapes.PT_CASES))
def test_the_far_end_rounds_accept_refuse_and_differ(name):
    zero = shapes.far_run(name, "zero")
    for position in ("straddle", "end"):
        r = shapes.far_run(name, position)
        acc, att = r.twin.book.accepts.sum(), r.twin.book.attempts.sum()
        print(f"{name} {position}: {int(acc)} of {int(att)} swaps accepted")
        assert 0 < acc < att
        assert (r.start == zero.start).all() and (r.twin.planes != zero.twin.planes).any()
        assert (r.rows_of(0, 1)[0] != zero.rows_of(0, 1)[0]).any()  # already the first round's sweeps differ
        assert (r.twin.book.accepts != zero.twin.book.accepts).any()
    s1, r1 = shapes.FAR_POSITIONS["end"]
    end = shapes.far_run(name, "end")
    assert end.twin.sweeps == 2 ** 31 and end.twin.book.rounds == 2 ** 32

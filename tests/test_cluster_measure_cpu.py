"""Cluster-size records on the host (no GPU needed): the new header and ctypes prototypes, the Python-integer twin
(tests/helpers/cluster_measure_twin.py) against brute-force counts, the 128-bit word join and cluster_estimators, the scans'
validation, and the improved estimator of <M^2> on the twin alone against full enumeration."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mtwin = _load("cluster_measure_twin")
lat3 = _load("lattice3d_twin")

NEW_SYMBOLS = ("tsu_ising2d_cluster_measure", "tsu_ising3d_cluster_measure", "tsu_ising2d_cluster_record", "tsu_ising3d_cluster_record")


def test_header_is_included_after_the_last_family_header():
    with open(os.path.join(ROOT, "include", "tsu_hip.h")) as f:
        top = f.read()
    assert re.search(r'^#include "tsu_hip_cluster_measure.h"', top, flags=re.M)
    others = [m.start() for m in re.finditer(r'^#include "tsu_hip_\w+\.h"', top, flags=re.M)]
    assert max(others) == top.index('#include "tsu_hip_cluster_measure.h"')
    # tsu_hip.h itself declares none of them: the ABI test compares its own declarations with _hip.SIGNATURES one to one
    assert not any(re.search(r"\b" + n + r"\s*\(", re.sub(r"/\*.*?\*/", "", top, flags=re.S)) for n in NEW_SYMBOLS)
    with open(os.path.join(ROOT, "tsu-emulator_amd", "csrc", "build.sh")) as f:
        assert "tsu_hip_cluster_measure.h" in f.read()


def test_symbols_are_exported_and_prototyped_one_to_one():
    from tsu import _hip
    with open(os.path.join(ROOT, "include", "tsu_hip_cluster_measure.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(tsu_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(NEW_SYMBOLS) == sorted(_hip.CLUSTER_MEASURE_SIGNATURES)
    lib = _hip.load_library()
    for name in NEW_SYMBOLS:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert len([a for a in proto.split(",") if a.strip()]) == len(_hip.CLUSTER_MEASURE_SIGNATURES[name][1]), name
        assert getattr(lib, name).argtypes == _hip.CLUSTER_MEASURE_SIGNATURES[name][1]
        assert getattr(lib, name).restype is _hip.CLUSTER_MEASURE_SIGNATURES[name][0]
    assert re.search(r"#define\s+TSU_CLUSTER_RECORD_WORDS\s+8\b", header) and _hip.CLUSTER_RECORD_WORDS == 8
    # disjoint from every other family dictionary, SIGNATURES included
    families = {k: v for k, v in vars(_hip).items() if k.endswith("SIGNATURES") and isinstance(v, dict)}
    assert len(families) >= 14 and "CLUSTER_MEASURE_SIGNATURES" in families
    for k, v in families.items():
        if k != "CLUSTER_MEASURE_SIGNATURES":
            assert not set(v) & set(NEW_SYMBOLS), k
    for cls in (_hip.Lattice, _hip.Lattice3D):
        assert callable(cls.cluster_measure) and callable(cls.cluster_record)


def _brute(roots, spins, frozen=None):
    """The row by a double loop over sites: no dictionaries, no NumPy reductions."""
    r, s = list(np.asarray(roots).ravel()), list(np.asarray(spins).ravel())
    fz = [x < 0 for x in r] if frozen is None else [bool(f) or x < 0 for f, x in zip(np.asarray(frozen).ravel(), r)]
    out = dict.fromkeys(mtwin.FIELDS, 0)
    for i in range(len(r)):
        if fz[i]:
            out["n_frozen"] += 1
            out["m_frozen"] += int(s[i])
        elif all(r[k] != r[i] or fz[k] for k in range(i)):  # the first site of its cluster
            members = [k for k in range(len(r)) if r[k] == r[i] and not fz[k]]
            size, m = len(members), sum(int(s[k]) for k in members)
            out["n_clusters"] += 1
            out["largest"] = max(out["largest"], size)
            out["sum_size2"] += size ** 2
            out["sum_m2"] += m ** 2
            out["sum_m4"] += m ** 4
    return out


def test_twin_record_against_brute_force_on_hand_made_labels():
    # one cluster of aligned spins
    one = mtwin.record(np.zeros((2, 3), int), np.ones((2, 3), int))
    assert one == _brute(np.zeros((2, 3), int), np.ones((2, 3), int))
    assert one == {"n_clusters": 1, "largest": 6, "sum_size2": 36, "sum_m2": 36, "sum_m4": 1296, "n_frozen": 0, "m_frozen": 0}
    # all singletons: every word counts sites
    s = np.array([1, -1, -1, 1, 1])
    single = mtwin.record(np.arange(5), s)
    assert single == _brute(np.arange(5), s)
    assert single == {"n_clusters": 5, "largest": 1, "sum_size2": 5, "sum_m2": 5, "sum_m4": 5, "n_frozen": 0, "m_frozen": 0}
    # two clusters with mixed spins (an antiferromagnetic bond joins opposite spins): M_C is signed and is not |C|
    roots = np.array([0, 0, 0, 3, 3, 0, 3])
    s = np.array([1, -1, 1, -1, -1, 1, 1])
    two = mtwin.record(roots, s)
    assert two == _brute(roots, s)
    assert two == {"n_clusters": 2, "largest": 4, "sum_size2": 16 + 9, "sum_m2": 4 + 1, "sum_m4": 16 + 1, "n_frozen": 0, "m_frozen": 0}
    # a frozen component, by root -1 and by the flag of cluster_field_twin.labels (whose roots stay site indices)
    roots = np.array([-1, 1, -1, 1, 4, -1])
    s = np.array([1, 1, -1, 1, -1, 1])
    fz = mtwin.record(roots, s)
    assert fz == _brute(roots, s)
    assert fz == {"n_clusters": 2, "largest": 2, "sum_size2": 5, "sum_m2": 5, "sum_m4": 17, "n_frozen": 3, "m_frozen": 1}
    flagged = np.array([0, 1, 0, 1, 4, 0])
    assert mtwin.record(flagged, s, frozen=flagged == 0) == fz == _brute(flagged, s, frozen=flagged == 0)
    rng = np.random.default_rng(1)
    for _ in range(20):
        roots = rng.integers(-1, 6, size=17)
        s = rng.choice([-1, 1], size=17)
        assert mtwin.record(roots, s) == _brute(roots, s)


def test_word_join_and_estimators_above_two_to_the_64():
    from tsu import _hip
    from tsu.models import ising
    N = 69632
    big = {"n_clusters": 1, "largest": N, "sum_size2": N ** 2, "sum_m2": N ** 2, "sum_m4": N ** 4, "n_frozen": 0, "m_frozen": 0}
    odd = {"n_clusters": 3, "largest": 50000, "sum_size2": 50000 ** 2 + 2, "sum_m2": 49999 ** 2 + 1, "sum_m4": 49999 ** 4 + 1 + 2 ** 127,
           "n_frozen": 19630, "m_frozen": -19630}
    assert N ** 4 > 2 ** 64
    rows = np.array([mtwin.words(big), mtwin.words(odd)], np.int64)
    assert rows[0, 5] == N ** 4 >> 64 and rows[0, 5] > 0 and rows[1, 5] < 0  # the high words; bit 127 reads back negative as int64
    rec = _hip.cluster_record_dict(rows)
    assert rec["sum_m4"].dtype == object and list(rec["sum_m4"]) == [big["sum_m4"], odd["sum_m4"]]
    assert all(type(v) is int for v in rec["sum_m4"])
    for k in mtwin.FIELDS:
        assert list(rec[k]) == [big[k], odd[k]], k
    rec["n_spins"] = N
    est = ising.cluster_estimators(rec)
    assert est["m2"][0] == 1.0 and est["m4"][0] == 1.0 and est["m"][0] == 0.0 and est["mean_cluster_size"][0] == float(N)
    # exact: the integers are combined before the one division, not as float64 products (N^4 is no float64 integer sum here)
    assert est["m2"][1] == (odd["sum_m2"] + odd["m_frozen"] ** 2) / N ** 2
    assert est["m"][1] == -19630 / N and math.isnan(est["m4"][1])  # M^4 is a zero-field estimator
    want = (3 * (7 ** 2 + 3 ** 2) ** 2 - 2 * (7 ** 4 + 3 ** 4)) / 10 ** 4
    got = ising.cluster_estimators({"n_spins": 10, "sum_m2": [58], "sum_m4": [7 ** 4 + 3 ** 4], "m_frozen": [0], "n_frozen": [0],
                                    "sum_size2": [58]})
    assert got["m4"][0] == want and got["mean_cluster_size"][0] == 5.8
    # the two-cluster identity itself: the mean of (e1 7 + e2 3)^4 over the four sign choices
    assert want * 10 ** 4 == sum((a * 7 + b * 3) ** 4 for a in (-1, 1) for b in (-1, 1)) / 4


def test_improved_needs_a_cluster_algorithm():
    from tsu import _hip
    from tsu.models import ising
    with pytest.raises(_hip.UnsupportedError, match="improved=True needs"):
        ising.temperature_scan(8, [2.0], improved=True, algorithm="gibbs")
    with pytest.raises(_hip.UnsupportedError, match="improved=True needs"):
        ising.temperature_scan_3d(4, [4.0], improved=True)
    with pytest.raises(ValueError, match="algorithm"):
        ising.temperature_scan_3d(4, [4.0], improved=True, algorithm="wolff")


def _batch_error(x, n_batches=20):
    x = np.asarray(x, dtype=np.float64)
    b = x[: len(x) // n_batches * n_batches].reshape(n_batches, -1).mean(axis=1)
    return float(b.std(ddof=1) / math.sqrt(n_batches))


def _exact_m2(n_sites, energy_of, T):
    E = np.array([energy_of(np.where((k >> np.arange(n_sites)) & 1, 1, -1)) for k in range(1 << n_sites)])
    M = np.array([2 * bin(k).count("1") - n_sites for k in range(1 << n_sites)], dtype=np.float64)
    w = np.exp(-(E - E.min()) / T)
    return float(np.sum(w * M ** 2) / np.sum(w))


def test_twin_improved_m2_against_enumeration():
    """<sum_m2> over 3000 twin steps after 100 discarded, against <M^2> of the full enumeration, within 4 batch-means errors
    (20 batches): open 3 x 3, J = 1, T = 2.0 and open 2 x 2 x 2, Gaussian couplings, T = 2.0."""
    T = 2.0
    s, _ = mtwin.sweep_2d(np.ones((3, 3), np.int8), False, 1.0, T, 100, 21)
    _, recs = mtwin.sweep_2d(s, False, 1.0, T, 3000, 21, step0=100)
    x = [r["sum_m2"] for r in recs]

    def e2(v):
        g = v.reshape(3, 3)
        return -float(np.sum(g[:, :-1] * g[:, 1:]) + np.sum(g[:-1, :] * g[1:, :]))
    exact = _exact_m2(9, e2, T)
    err = _batch_error(x)
    print(f"\n3x3: <sum_m2> = {np.mean(x):.4f} +- {err:.4f}, exact <M^2> = {exact:.4f}")
    assert abs(np.mean(x) - exact) < 4 * err

    shape = (2, 2, 2)
    jr, jd, jl, _ = lat3.enumeration_disorder(shape, 3)
    s, _ = mtwin.sweep_3d(np.ones(shape, np.int8), False, jr, jd, jl, T, 100, 11)
    _, recs = mtwin.sweep_3d(s, False, jr, jd, jl, T, 3000, 11, step0=100)
    x = [r["sum_m2"] for r in recs]
    exact = _exact_m2(8, lambda v: lat3.energy(v.reshape(shape), False, jr, jd, jl), T)
    err = _batch_error(x)
    print(f"2x2x2: <sum_m2> = {np.mean(x):.4f} +- {err:.4f}, exact <M^2> = {exact:.4f}")
    assert abs(np.mean(x) - exact) < 4 * err

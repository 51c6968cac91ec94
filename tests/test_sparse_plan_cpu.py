"""K5's route choice without a GPU: tsu_sparse_classify (the validation and classifier of tsu_sparse_create as pure host code) against
the NumPy twin written from the classifier's rules (tests/helpers/sparse_plan_twin.py) and against literal plans, on the graphs that
tests/test_sparse_routes_gpu.py then sweeps."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tsu-emulator_amd"))
from tsu import _hip  # noqa: E402
from tsu.graph import canonical_csr, color_graph  # noqa: E402

_spec = importlib.util.spec_from_file_location("sparse_plan_twin", os.path.join(HERE, "helpers", "sparse_plan_twin.py"))
twin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(twin)

# (graph, n): the table of the route tests
TABLE = ([(g, n) for g in ("dimers", "degree3", "degree4", "asymmetric", "halves") for n in (40008, 40010)]
         + [("strip", 30000), ("strip", 30006), ("strip", 60000), ("strip", 60006)]
         + [(g, 40008) for g in ("chain", "chain_first38", "chain_first64", "chain_first65", "chain_both_ends", "chain_interior",
                                 "chain_descending")]
         + [("chain_odd_first", 40009)])
SUPPLIED_ORDER = ("strip", "chain_odd_first", "chain_descending")


def _classify(A, bias, offsets, order):
    return _hip.sparse_classify(A.indptr, A.indices, A.data, bias, offsets, order)


@pytest.mark.parametrize("name,n", TABLE)
@pytest.mark.parametrize("pair", [1, 0])
def test_classifier_equals_twin_and_literal_plan(name, n, pair, monkeypatch):
    monkeypatch.setenv("TSU_K5_PAIR", str(pair))
    for k in ("TSU_K5_STENCIL", "TSU_K5_V4"):
        monkeypatch.delenv(k, raising=False)
    A, bias, offsets, order, classes, pairs = twin.graph(name, n)
    if name not in SUPPLIED_ORDER:  # the colouring the package itself would choose
        off2, ord2 = color_graph(A)
        np.testing.assert_array_equal(off2, offsets)
        np.testing.assert_array_equal(ord2, order)
    got = _classify(A, bias, offsets, order)
    assert got == twin.classify(A.indptr, A.indices, A.data, bias, offsets, order, use_pairs=bool(pair))
    assert got == twin.expected_plan(offsets, classes, pairs, use_pairs=bool(pair))


def test_literal_plans_of_the_table():
    """The values themselves, spelled out once more without the helper's record builder: (deg, lo, hi, site_stride), pair, v4."""
    def short(name, n):
        A, bias, offsets, order, _, _ = twin.graph(name, n)
        return [(r["route"], r["deg"], r["lo"], r["hi"], r["site_stride"], r["pair"], r["v4"]) for r in _classify(A, bias, offsets, order)]
    assert short("dimers", 40008) == [(1, 1, 0, 0, 2, 1, 1), (1, 1, 0, 0, 2, 2, 1)]
    assert short("dimers", 40010) == [(1, 1, 0, 0, 2, 1, 0), (1, 1, 0, 0, 2, 2, 0)]       # the second class starts at 20005
    assert short("degree3", 40008) == [(1, 3, 1, 1, 2, 1, 1), (1, 3, 1, 1, 2, 2, 1)]
    assert short("degree4", 40008) == [(1, 4, 2, 1, 2, 1, 1), (1, 4, 1, 2, 2, 2, 1)]
    assert short("asymmetric", 40008) == [(1, 4, 2, 1, 2, 1, 1), (1, 2, 0, 1, 2, 2, 1)]
    assert short("halves", 40008) == [(1, 2, 1, 0, 1, 0, 1), (1, 2, 0, 1, 1, 0, 1)]       # stride 1: no pair
    assert short("halves", 40010) == [(1, 2, 1, 0, 1, 0, 1), (1, 2, 0, 1, 1, 0, 0)]
    # (the strip's classes are regular at any size, but up to 32768 sites the whole system runs on k5_small: route 2, v4 0)
    assert short("strip", 30000) == [(2, 4, 1, 0, 3, 0, 0), (2, 4, 1, 1, 3, 0, 0), (2, 4, 0, 1, 3, 0, 0)]
    assert short("strip", 30006) == [(2, 4, 1, 0, 3, 0, 0), (2, 4, 1, 1, 3, 0, 0), (2, 4, 0, 1, 3, 0, 0)]
    assert short("strip", 60000) == [(1, 4, 1, 0, 3, 0, 1), (1, 4, 1, 1, 3, 0, 1), (1, 4, 0, 1, 3, 0, 1)]
    assert short("strip", 60006) == [(1, 4, 1, 0, 3, 0, 1), (1, 4, 1, 1, 3, 0, 0), (1, 4, 0, 1, 3, 0, 1)]  # classes at 20002, 40004
    assert short("chain_first38", 40008) == [(1, 2, 38, 0, 2, 1, 1), (1, 2, 0, 1, 2, 2, 1)]
    assert short("chain_first64", 40008) == [(1, 2, 64, 0, 2, 1, 1), (1, 2, 0, 1, 2, 2, 1)]
    assert short("chain_first65", 40008) == [(0, 0, 0, 0, 0, 0, 0), (1, 2, 0, 1, 2, 0, 1)]  # 65 rows: one more than K5_EDGE
    assert short("chain_both_ends", 40008) == [(1, 2, 3, 0, 2, 1, 1), (1, 2, 0, 61, 2, 2, 1)]
    assert short("chain_interior", 40008) == [(0, 0, 0, 0, 0, 0, 0), (1, 2, 0, 1, 2, 0, 1)]
    assert short("chain_odd_first", 40009) == [(1, 2, 0, 0, 2, 1, 1), (1, 2, 1, 1, 2, 2, 1)]
    assert short("chain_descending", 40008) == [(1, 2, 0, 1, -2, 0, 1), (1, 2, 1, 0, -2, 0, 1)]
    # the partner's rows as the first class of a pair sees them
    A, bias, offsets, order, _, _ = twin.graph("chain_both_ends", 40008)
    r = _classify(A, bias, offsets, order)
    assert (r[0]["other"], r[0]["o_lo"], r[0]["o_n"], r[1]["other"], r[1]["o_n"]) == (1, 0, 20004 - 61, 0, 0)
    A, bias, offsets, order, _, _ = twin.graph("chain_odd_first", 40009)
    r = _classify(A, bias, offsets, order)
    assert offsets[2] - offsets[1] == offsets[1] + 1 and (r[0]["o_lo"], r[0]["o_n"]) == (1, 20003)  # the second class is one longer


def _existing(shape, n):
    """chain, ring and ladder as tests/test_sparse_gpu.py builds them."""
    if shape == "chain":
        A = canonical_csr(sp.diags([np.full(n - 1, 0.8), np.full(n - 1, 0.8)], [1, -1]))
    elif shape == "ring":
        A = canonical_csr(sp.diags([np.full(n - 1, 0.8), np.full(n - 1, 0.8), [0.8], [0.8]], [1, -1, n - 1, -(n - 1)]))
    else:
        L = n // 2
        i = np.arange(L - 1)
        rows = np.concatenate([2 * i, 2 * i + 1, 2 * np.arange(L)])
        cols = np.concatenate([2 * i + 2, 2 * i + 3, 2 * np.arange(L) + 1])
        B = sp.coo_matrix((np.full(rows.size, -0.6), (rows, cols)), shape=(n, n))
        A = canonical_csr(B + B.T)
    return A, np.full(n, 0.3)


@pytest.mark.parametrize("shape,n", [("chain", 300001), ("ring", 100000), ("ladder", 80000), ("chain", 4099)])
def test_existing_shapes(shape, n, monkeypatch):
    for k in ("TSU_K5_STENCIL", "TSU_K5_V4", "TSU_K5_PAIR"):
        monkeypatch.delenv(k, raising=False)
    A, bias = _existing(shape, n)
    offsets, order = color_graph(A)
    got = _classify(A, bias, offsets, order)
    assert got == twin.classify(A.indptr, A.indices, A.data, bias, offsets, order)
    routes = [r["route"] for r in got]
    if n == 4099:
        assert routes == [2, 2] and [r["v4"] for r in got] == [0, 0]
    elif shape == "ladder":
        # class 0 holds sites 0, 3, 4, 7, 8, ...: the site number is not affine in the position, no row fits
        assert routes == [0, 0]
    else:
        assert routes == [1, 1] and [r["deg"] for r in got] == [2, 2] and [r["pair"] for r in got] == [1, 2]


def test_switches_are_read_when_a_graph_is_classified(monkeypatch):
    A, bias, offsets, order, classes, pairs = twin.graph("chain", 40008)
    args = (A.indptr, A.indices, A.data, bias, offsets, order)
    monkeypatch.setenv("TSU_K5_V4", "0")
    assert _classify(A, bias, offsets, order) == twin.classify(*args, use_v4=False) == twin.expected_plan(offsets, classes, pairs, use_v4=False)
    monkeypatch.setenv("TSU_K5_STENCIL", "0")
    assert [r["route"] for r in _classify(A, bias, offsets, order)] == [0, 0]
    assert _classify(A, bias, offsets, order) == twin.classify(*args, use_stencil=False)


def test_classify_validates_like_create():
    A, bias, offsets, order, _, _ = twin.graph("chain", 40008)
    with pytest.raises(ValueError, match="same colour"):
        _classify(A, bias, offsets, np.arange(40008))
    bad = order.copy()
    bad[-1] = bad[0]
    with pytest.raises(ValueError, match="permutation"):
        _classify(A, bias, offsets, bad)
    with pytest.raises(ValueError, match="offsets"):
        _classify(A, bias, np.array([0, 20004, 40007], np.int32), order)
    assert _classify(A, None, offsets, order)[0]["route"] == 1  # no bias: zeros

"""K1 periodic byte-plane tiles with the thresholds of four sites per LDS read (the 625-entry table and the up-flags stored as 8:
pair_thresholds in ising2d_tiled.hip): every loop form that takes the table -- plain, EDGE and SEAM, launch-per-generation and
tile-resident -- against the generic kernel, bit for bit, spins and observables.  The comparison and the case format are those of
test_k1_pair_table_gpu.py; the child (tests/helpers/k1_quad_table_check.py) adds the start, the index tally and a table.

Shapes: the smallest that run each form.  Variant 2 is the benchmark's tile shape (128 x 512 sites, 1024 threads): 256 rows are two
tiles whose windows both hold the wrap row of a height that is a power of two (plain loop), 384 rows are three tiles of which two
hold the wrap row of a height that is not (EDGE); 500 columns leave a ragged last octet (SEAM); a slab from row 383 starts its
windows on an odd row (the other column parity).  Variant 7 has the narrow tiles (NO = 18).  An open lattice (v_perm tables) and
nibble planes (variant 8, the 25-entry table) are the controls that the forms which keep 0 / 1 flags still agree.

Tables: the critical temperature's; "coarse", whose thresholds tie with the top 16 random bits often (the tie path takes the counts
scaled by 8); "field", asymmetric; "clamp_reversed", both ends of the signed 16-bit range, not monotonic in the count; "distinct",
five thresholds 0.2 of the range apart in no order, so that a threshold from another position of an entry or an entry found with
a wrong weight changes accepts.

Inputs: of the 625 index values c0 + 5 c1 + 25 c2 + 125 c3, 479 can occur (neighbouring sites share a spin: no 4 beside a 0).
Every byte-plane periodic case must meet all 479 in the count dwords of the half-sweeps that start its calls, counted by the child
from the generic kernel's states; the start plants them (see the child).

Every launch must report the threshold form it ran with (TSU_K1_VERBOSE=1): the quad table on periodic byte planes, the pair table
on nibble planes, v_perm on the open lattice."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = [24, 21]
TABLES = ["tc", "coarse", "field", "clamp_reversed", "distinct"]


def resident(rows, cols, k, tiles, **more):
    return dict(rows=rows, cols=cols, k=k, calls=CALLS, one_launch=True, tiles=tiles, all_indices=True, **more)


# variant (index of the tile shape table in ising2d_tiled.hip), threshold form of its periodic launches, cases
GROUPS = {
    "32x256_T1024": (7, "quad table", [resident(128, 256, 1, 4), resident(128, 256, 8, 4, table="distinct")]),
    "128x512_T1024_tables": (2, "quad table", [resident(256, 512, 8, 2, table=t) for t in TABLES] + [resident(256, 512, 5, 2, table="distinct")]),
    "128x512_T1024_forms": (2, "quad table", [
        resident(384, 512, 8, 3, table="distinct"),                          # EDGE
        resident(384, 512, 8, 3, table="coarse"),
        dict(rows=384, cols=500, k=8, calls=CALLS, all_indices=True, table="distinct"),  # SEAM
        dict(rows=384, cols=500, k=8, calls=CALLS, all_indices=True, table="coarse"),
        dict(rows=512, cols=512, k=8, calls=[16, 16], slab=[383, 128, 32], all_indices=True, table="distinct"),  # windows from an odd row
        dict(rows=512, cols=512, k=8, calls=[16, 16], slab=[383, 128, 32], all_indices=True, table="coarse"),
        dict(rows=384, cols=512, k=8, calls=[8, 5], all_indices=True, table="distinct"),  # a launch per generation
        dict(rows=383, cols=500, k=8, calls=CALLS, periodic=False, table="distinct"),     # open: the v_perm form, 0 / 1 flags
    ]),
    "128x512_T1024_renumber": (2, "quad table", [dict(rows=256, cols=512, k=1, renumber=True, call=1000, table="distinct")]),
    "nib_512x512_T1024": (8, "pair table", [dict(rows=2048, cols=512, k=8, calls=CALLS, one_launch=True, tiles=4, table="distinct")]),
}


def launches_of(stderr):
    """case index -> [(kernel, variant, threshold form)] of its tiled launches, and -> [(variant, tiles, generations, sweeps per
    generation)] of the tile-resident ones (TSU_K1_VERBOSE=1)"""
    forms, res, case = {}, {}, None
    for line in stderr.splitlines():
        m = re.match(r"\[case (\d+)\]", line)
        if m:
            case = int(m.group(1))
            forms[case], res[case] = [], []
        m = re.match(r"\[tsu\] (k1_resident|k1_tiled2) variant (\d+): .*thresholds: ([a-z_ ]+?)(?:, row wrap: \w+)?$", line)
        if m:
            forms[case].append((m.group(1), int(m.group(2)), m.group(3)))
        m = re.match(r"\[tsu\] k1_resident variant (\d+): (\d+) tiles .*, (\d+) generations of (\d+) sweeps", line)
        if m:
            res[case].append(tuple(int(g) for g in m.groups()))
    return forms, res


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_quad_table_compare_equals_the_generic_kernel(group):
    variant, periodic_form, cases = GROUPS[group]
    env = dict(os.environ, TSU_TILE_VARIANT=str(variant), TSU_K1_VERBOSE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "k1_quad_table_check.py"), json.dumps(cases)], env=env,
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("\nok ") + r.stdout.startswith("ok ") == len(cases)
    forms, res = launches_of(r.stderr)
    for index, case in enumerate(cases):
        # the forced shape was taken, with the threshold form this test is about
        want = periodic_form if case.get("periodic", True) else "v_perm"
        assert forms.get(index) and all(v == variant and f == want for _, v, f in forms[index]), (case, forms.get(index))
        if "tiles" in case:
            k = case["k"]
            assert res[index] == [(variant, case["tiles"], -(-n // k), k) for n in case["calls"]], (case, res[index])
        if case.get("renumber"):
            assert res[index] and all(kern == "k1_resident" for kern, _, _ in forms[index]), (case, forms[index])

"""K1 periodic tiles with the pair thresholds from the 25-entry LDS table (pair_thresholds in ising2d_tiled.hip): every loop form
that takes the table -- plain, EDGE and SEAM, byte and nibble planes, launch-per-generation and tile-resident -- against the generic
kernel, bit for bit, spins and observables.  The comparison and the case format are those of test_k1_interleaved_planes_gpu.py; the
child (tests/helpers/k1_pair_table_check.py) adds threshold tables.

Shapes: the smallest that run each form.  Variant 2 is the benchmark's tile shape (128 x 512 sites, 1024 threads): 256 rows are two
tiles whose windows both hold the wrap row of a height that is a power of two (plain loop, the wrap in the Philox head), 384 rows are
three tiles of which two hold the wrap row of a height that is not (EDGE); 500 columns leave a ragged last octet (SEAM); a slab from
row 383 starts its windows on an odd row (the other column parity).  Variant 7 has the narrow tiles (NO = 18), variants 8 and 9 the
nibble planes.  An open lattice is the control that the v_perm form, which open lattices keep, still agrees.

Tables (the table index is c0 + 5 c1 for the counts of a site pair; a random start reaches all 25 pairs in the first half-sweep at
these sizes): the critical temperature's; "coarse", whose thresholds tie with the top 16 random bits often (the tie path behind the
new compare); "field", five distinct asymmetric entries, so that a swapped (c0, c1) or a wrong weight shows; "clamp", both ends of
the signed 16-bit range of the stored fields and the 65535 clamp; "clamp_reversed", not monotonic in the count."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = [24, 21]
TABLES = ["tc", "coarse", "field", "clamp", "clamp_reversed"]


def resident(rows, cols, k, tiles, **more):
    return dict(rows=rows, cols=cols, k=k, calls=CALLS, one_launch=True, tiles=tiles, **more)


# variant (index of the tile shape table in ising2d_tiled.hip), cases
GROUPS = {
    "32x256_T1024": (7, [resident(128, 256, 1, 4), resident(128, 256, 8, 4)]),
    "128x512_T1024": (2, [resident(256, 512, 8, 2, table=t) for t in TABLES] + [
        resident(256, 512, 5, 2),
        resident(384, 512, 8, 3),                                        # EDGE
        resident(384, 512, 8, 3, table="field"),
        dict(rows=512, cols=512, k=8, calls=[16, 16], slab=[383, 128, 32]),  # windows from an odd row
        dict(rows=512, cols=512, k=8, calls=[16, 16], slab=[383, 128, 32], table="clamp"),
        dict(rows=384, cols=512, k=8, calls=[8, 5]),                     # a launch per generation
        dict(rows=384, cols=500, k=8, calls=CALLS),                      # SEAM
        dict(rows=384, cols=500, k=8, calls=CALLS, table="field"),
        dict(rows=383, cols=500, k=8, calls=CALLS, periodic=False),      # open: the v_perm form
        dict(rows=383, cols=500, k=8, calls=CALLS, periodic=False, table="field"),
    ]),
    "nib_512x512_T1024": (8, [resident(2048, 512, 8, 4, table=t) for t in TABLES] + [
        dict(rows=2048, cols=500, k=8, calls=CALLS, table="field"),      # SEAM on nibble planes
    ]),
    "nib_256x512_T512": (9, [dict(rows=1024, cols=512, k=8, calls=CALLS, table=t) for t in ("tc", "field", "clamp_reversed")]),
}


def resident_launches(stderr):
    """case index -> [(variant, tiles, generations, sweeps per generation)] of its tile-resident launches (TSU_K1_VERBOSE=1)"""
    out, case = {}, None
    for line in stderr.splitlines():
        m = re.match(r"\[case (\d+)\]", line)
        if m:
            case = int(m.group(1))
            out[case] = []
        m = re.match(r"\[tsu\] k1_resident variant (\d+): (\d+) tiles .*, (\d+) generations of (\d+) sweeps", line)
        if m:
            out[case].append(tuple(int(g) for g in m.groups()))
    return out


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_table_compare_equals_the_generic_kernel(group):
    variant, cases = GROUPS[group]
    env = dict(os.environ, TSU_TILE_VARIANT=str(variant), TSU_K1_VERBOSE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "k1_pair_table_check.py"), json.dumps(cases)], env=env,
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("\nok ") + r.stdout.startswith("ok ") == len(cases)
    # the forced shape was taken: every tile-resident launch reports the variant, and where the case names it the number of tiles
    # and the cut into generations
    launches = resident_launches(r.stderr)
    for index, case in enumerate(cases):
        got = launches.get(index, [])
        assert all(v == variant for v, _, _, _ in got), (case, got)
        if "tiles" in case:
            k = case["k"]
            assert got == [(variant, case["tiles"], -(-n // k), k) for n in case["calls"]], (case, got)

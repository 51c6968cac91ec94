"""K1 tiles on lattices whose height is a power of two: the periodic row wrap is taken in the first Philox XOR (the row counter
of the pair loop runs on past the last row and the head computes (row & (rows - 1)) ^ y0), so the tiles whose windows hold the
wrap row run the plain pair loop.  Every case against the generic kernel, bit for bit, spins and observables, through
tests/helpers/k1_layout_check.py (one child process per forced tile shape, as in test_k1_interleaved_planes_gpu.py).

The smallest shapes at which the mask can go wrong:
  * 32 x 256 tiles on 128 rows: four tile rows, two of them wrap-holding; at k = 8 a window (TR = 64) is half the lattice.  On 64
    rows TR = rows: both windows hold the wrap and the unwrapped row counter reaches 2 rows - 1, the most the mask is asked to
    fold.  (Forced to the tiled kernel the 64 x 256 lattice stays on it: 64 = H + 4 KMAX rows is the least the shape takes.)
  * the bench shape (128 x 512 tiles, 1024 threads) on 512 and 256 rows (both tile rows hold the wrap); with the coarse table ties
    fall in the wrapped halo rows, whose low bits the tie path must draw from the masked row; row slabs of a 512-row lattice
    whose windows cross row 512, from an odd first row (the other column parity), tile-resident and launch per generation.
  * nibble planes: 512 x 512 tiles on 2048 rows (tile-resident), 256 x 512 tiles on 1024 rows (launch per generation).
  * control: 384 rows are no power of two and keep the EDGE loop's compares.

How the wrap is taken is read from the end of the library's TSU_K1_VERBOSE line of every tile-resident launch (launch-per-
generation calls report nothing)."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = [24, 21]

# variant (index of the tile shape table in ising2d_tiled.hip), the report every tile-resident launch must end with, cases
GROUPS = {
    "32x256_T1024": (7, "mask", [dict(rows=128, cols=256, k=k, calls=CALLS, one_launch=True) for k in (1, 5, 8)] + [
        dict(rows=64, cols=256, k=8, calls=CALLS, one_launch=True),      # TR = rows: rows up to 2 rows - 1 under the mask
    ]),
    "128x512_T1024": (2, "mask", [dict(rows=512, cols=512, k=k, calls=CALLS, one_launch=True) for k in (1, 5, 8)] + [
        dict(rows=256, cols=512, k=8, calls=CALLS, one_launch=True),     # both tile rows hold the wrap
        dict(rows=256, cols=512, k=8, calls=CALLS, one_launch=True, table="coarse"),  # ties in wrapped halo rows
        dict(rows=512, cols=512, k=8, calls=[16, 16], slab=[383, 128, 32], one_launch=True),  # odd first row, window crosses row 512
        dict(rows=512, cols=512, k=8, calls=[8, 5], slab=[384, 128, 16]),   # launch per generation
    ]),
    "nib_512x512_T1024": (8, "mask", [dict(rows=2048, cols=512, k=k, calls=CALLS, one_launch=True) for k in (5, 8)] + [
        dict(rows=2048, cols=512, k=8, calls=CALLS, one_launch=True, table="coarse"),
    ]),
    "nib_256x512_T512": (9, "mask", [dict(rows=1024, cols=512, k=8, calls=CALLS)]),
    "128x512_T1024_control": (2, "compare", [dict(rows=384, cols=512, k=8, calls=CALLS, one_launch=True)]),
}


def resident_reports(stderr):
    """case index -> [(variant, how the row wrap is taken)] of its tile-resident launches (TSU_K1_VERBOSE=1)"""
    out, case = {}, None
    for line in stderr.splitlines():
        m = re.match(r"\[case (\d+)\]", line)
        if m:
            case = int(m.group(1))
            out[case] = []
        m = re.match(r"\[tsu\] k1_resident variant (\d+): .*, row wrap: (\w+)$", line)
        if m:
            out[case].append((int(m.group(1)), m.group(2)))
    return out


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_row_mask_equals_the_generic_kernel(group):
    variant, wrap, cases = GROUPS[group]
    env = dict(os.environ, TSU_TILE_VARIANT=str(variant), TSU_K1_VERBOSE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "k1_layout_check.py"), json.dumps(cases)], env=env,
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    print(r.stderr[-3000:])
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("\nok ") + r.stdout.startswith("ok ") == len(cases)
    reports = resident_reports(r.stderr)
    for index, case in enumerate(cases):
        got = reports.get(index, [])
        # a tile-resident case reports once per call, a launch-per-generation case never
        assert len(got) == (len(case["calls"]) if case.get("one_launch") else 0), (case, got)
        assert all(g == (variant, wrap) for g in got), (case, got)

"""K1 tiles with the two colour planes interleaved row by row in LDS and the pair loop on one induction pointer: every form of the
loop (plain, EDGE, SEAM, OPEN; byte and nibble planes; launch-per-generation and tile-resident) against the generic kernel, bit
for bit, spins and observables.

Per tile shape the smallest lattice with three tile rows and one tile column: one interior tile row (plain loop) and the two whose
windows hold the lattice's wrap row (EDGE).  Calls of 24 and 21 sweeps: full generations of k sweeps plus a short last one;
k = 1, 5 and 8 move the halo depth, hence every immediate row offset's meaning and the trip counts.  The row stride (2 NO octets)
and the plane distance (NO octets) depend on the tile width (NO = 34 or 18 octets) and the octet size (8 bytes, 4 on nibble planes)
only, so each of the ten shapes' own lattice covers them for any height.

Trip counts: a half-sweep of P row pairs on RL row lanes runs P // RL iterations on every lane and a last one on the first
P % RL row lanes.  With 1024 threads and 34 octets RL = 30; three flexible tile rows of 118 rows at k = 1 have P = 60 in the first
half-sweep of a generation (no lane has a last iteration: every wave skips it) and P = 59 in the second (29 of the 30 row lanes
have one, the most there can be); the standard shapes at k = 8 run through 16 consecutive P.

The column parity of a tile's first updated row is fixed per tile.  Whole lattices always have one value of it (their windows
start on even rows); the other needs a window that starts on an odd global row: a row slab whose first row is odd.

That a forced shape was taken is read from the library's TSU_K1_VERBOSE line of every tile-resident launch (variant, tiles,
generations): three tiles on the 354-row lattice are the three 118-row tiles of the trip-count case."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = [24, 21]


def std(rows, cols, one_launch):
    # three tile rows, one tile column
    return [dict(rows=rows, cols=cols, k=k, calls=CALLS, one_launch=one_launch, **({"tiles": 3} if one_launch else {})) for k in (1, 5, 8)]


# variant (index of the tile shape table in ising2d_tiled.hip), extra environment, cases
GROUPS = {
    "64x512_T512": (0, {}, std(192, 512, True)),
    "128x512_T512": (1, {}, std(384, 512, True)),
    "128x512_T1024": (2, {}, std(384, 512, True) + [
        dict(rows=384, cols=500, k=8, calls=CALLS),                     # periodic, ragged width: SEAM
        dict(rows=384, cols=500, k=5, calls=CALLS),
        dict(rows=383, cols=500, k=8, calls=CALLS, periodic=False),     # open, odd height, ragged width: OPEN
        dict(rows=383, cols=500, k=1, calls=CALLS, periodic=False),
        dict(rows=384, cols=512, k=8, calls=CALLS, table="coarse"),     # the tie path
        dict(rows=384, cols=512, k=8, calls=CALLS, table="coarse", periodic=False),
        # windows that start on an odd global row (the other column parity): slabs of 128 rows, launch per generation and
        # (ghost rows for two generations of 8 sweeps) tile-resident; the second slab's window holds the wrap row (EDGE)
        dict(rows=384, cols=512, k=8, calls=[8, 5], slab=[129, 128, 16]),
        dict(rows=384, cols=512, k=8, calls=[16, 16], slab=[129, 128, 32]),
        dict(rows=384, cols=512, k=4, calls=[12, 12], slab=[255, 128, 32]),
        dict(rows=384, cols=500, k=4, calls=[8, 7], slab=[255, 128, 16]),
    ]),
    "256x512_T1024": (3, {}, std(768, 512, True) + [
        dict(rows=383, cols=500, k=8, calls=CALLS, periodic=False),     # open, flexible cut into 16-row tiles, resident
    ]),
    "256x512_T1024_flex3": (3, {"TSU_K1_FLEX_MAX_TILES": "3"}, [
        dict(rows=388, cols=512, k=8, calls=CALLS, one_launch=True, tiles=3),    # tile rows of 128, 130 and 130 rows
        dict(rows=388, cols=512, k=5, calls=CALLS, one_launch=True, tiles=3),
        dict(rows=354, cols=512, k=1, calls=CALLS, one_launch=True, tiles=3),    # 118-row tiles: empty and full last iterations
        dict(rows=383, cols=500, k=8, calls=CALLS, periodic=False),     # open, three tile rows, the last one row short
    ]),
    "128x256_T1024": (4, {}, std(384, 256, True)),
    "64x512_T1024": (5, {}, std(192, 512, True)),
    "64x256_T1024": (6, {}, std(192, 256, True)),
    "32x256_T1024": (7, {}, std(96, 256, True)),
    "nib_512x512_T1024": (8, {}, std(1536, 512, True) + [
        dict(rows=1536, cols=500, k=8, calls=CALLS),                    # SEAM on nibble planes
        dict(rows=1535, cols=500, k=8, calls=CALLS, periodic=False),    # OPEN on nibble planes
        dict(rows=1536, cols=512, k=8, calls=CALLS, table="coarse"),
    ]),
    "nib_256x512_T512": (9, {}, std(768, 512, False) + [
        dict(rows=768, cols=500, k=8, calls=CALLS),
        dict(rows=767, cols=500, k=8, calls=CALLS, periodic=False),
    ]),
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
def test_tiles_equal_the_generic_kernel(group):
    variant, extra, cases = GROUPS[group]
    env = dict(os.environ, TSU_TILE_VARIANT=str(variant), TSU_K1_VERBOSE="1", **extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "k1_layout_check.py"), json.dumps(cases)], env=env,
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("\nok ") + r.stdout.startswith("ok ") == len(cases)
    # the forced shape was taken: every tile-resident launch reports the variant, and where the case names it the number of tiles
    # and the cut into generations (the library reports nothing for launch-per-generation calls: there the launch counts that
    # the child checks, one per generation, are all that shows)
    launches = resident_launches(r.stderr)
    for index, case in enumerate(cases):
        got = launches.get(index, [])
        assert all(v == variant for v, _, _, _ in got), (case, got)
        if "tiles" in case:
            k = case["k"]
            assert got == [(variant, case["tiles"], -(-n // k), k) for n in case["calls"]], (case, got)

"""Child process of tests/test_k1_pair_table_gpu.py: TSU_TILE_VARIANT is read once per process, so every forced tile shape gets
its own process.  The same cases and the same comparison as tests/helpers/k1_layout_check.py; what differs is the threshold tables.  Sweeps lattices (or one row slab of a lattice) on the tiled kernel and
compares spins and observables with the generic kernel (one thread per site, no tiles, no LDS), bit for bit.

A case is a JSON object: rows, cols, k (sweeps per generation), calls (sweeps of each call) and, optionally, periodic (default
true), table (see TABLES), one_launch (the tiles must stay resident: one launch per call), tiles (read by the parent test: the number of tiles the
resident launches must report) and slab = [row0, slab rows, ghost]: the tiled kernel then runs
on that slab of the lattice alone, its ghost rows refreshed from the generic kernel's lattice before every call."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))
import numpy as np  # noqa: E402
from tsu import _hip  # noqa: E402



def with_degree4(entries):
    """the critical temperature's table with its degree-4 row (the only one a periodic lattice reads) replaced"""
    t = _hip.ising2d_thresholds(1.0, 0.0, 2.269185).copy()
    t[20:25] = np.array(entries, dtype=np.uint64)
    return t


# the top 16 bits of a threshold enter the compare as min(thr >> 16, 65535) ^ 0x8000, a signed 16-bit number: CLAMP holds both
# ends of that range (0 -> -32768, 0x7FFF8000 -> -1, 1 << 16 -> -32767, 0xFFFF0000 -> 32767) and 2^32 ("always accept", the largest
# threshold a lattice takes), whose top bits, 65536, the 65535 clamp maps to 32767 as well
CLAMP = [0, 1 << 16, 0x7FFF8000, 0xFFFF0000, 1 << 32]
TABLES = {"tc": _hip.ising2d_thresholds(1.0, 0.0, 2.269185),
          # the tie-path table of test_ising2d_tiled_ties_and_clamps: low halves that tie often
          "coarse": np.array([(k * 0x0A3D) << 16 | 0x8000 for k in range(25)], dtype=np.uint64),
          # a field: five distinct, asymmetric degree-4 entries, so a swapped (c0, c1) index or a wrong weight shows
          "field": _hip.ising2d_thresholds(1.0, 0.3, 2.0),
          "clamp": with_degree4(CLAMP),
          "clamp_reversed": with_degree4(CLAMP[::-1])}   # not monotonic in the count


def fail(case, what):
    print(f"MISMATCH {json.dumps(case)}: {what}")
    sys.exit(1)


ctx = _hip.Context(0)
for index, case in enumerate(json.loads(sys.argv[1])):
    print(f"[case {index}]", file=sys.stderr, flush=True)  # the library's TSU_K1_VERBOSE lines of this case follow it on stderr
    rows, cols, k, calls = case["rows"], case["cols"], case["k"], case["calls"]
    periodic = case.get("periodic", True)
    table = TABLES[case.get("table", "tc")]
    ref = _hip.Lattice(rows, cols, periodic, ctx=ctx)
    ref.set_kernel(_hip.KERNEL_GENERIC, 0)
    ref.randomize(rows + cols)
    ref.set_thresholds(table)
    slab = case.get("slab")
    if slab:
        row0, own, ghost = slab
        lat = _hip.Lattice(own, cols, periodic, ctx=ctx, total_rows=rows, row0=row0, ghost=ghost)
    else:
        lat = _hip.Lattice(rows, cols, periodic, ctx=ctx)
        lat.randomize(rows + cols)
    lat.set_kernel(_hip.KERNEL_TILED, k)
    lat.set_thresholds(table)
    done, launches = 0, []
    for n in calls:
        if slab:  # owned rows and ghost rows from the whole lattice (the window wraps on a periodic one)
            full = ref.get_spins()
            window = np.arange(row0 - ghost, row0 + own + ghost)
            assert periodic or (window[0] >= 0 and window[-1] < rows)
            win = full[window % rows]
            lat.set_spins(win[:ghost], row_first=-ghost)
            lat.set_spins(win[ghost:ghost + own])
            lat.set_spins(win[ghost + own:], row_first=own)
        l0 = lat.launch_count()
        lat.sweep(n, 13, done)
        ref.sweep(n, 13, done)
        done += n
        launches.append(lat.launch_count() - l0)
        want = ref.get_spins()
        if slab:
            want = want[row0:row0 + own]
        got = lat.get_spins()
        if not (got == want).all():
            bad = np.argwhere(got != want)
            fail(case, f"after {done} sweeps {len(bad)} sites differ, first {bad[:5].tolist()}")
        if not slab and lat.observables() != ref.observables():
            fail(case, f"observables after {done} sweeps")
    if case.get("one_launch") and launches != [1] * len(calls):
        fail(case, f"not tile-resident: launches per call {launches}")
    print(f"ok {json.dumps(case)} launches={launches}", flush=True)
    lat.close()
    ref.close()
print("ALL OK")

"""Child process of tests/test_k1_quad_table_gpu.py: TSU_TILE_VARIANT is read once per process, so every forced tile shape gets
its own process.  Cases and comparison are those of tests/helpers/k1_pair_table_check.py: a lattice (or one row slab of a lattice)
swept on the tiled kernel against the generic kernel (one thread per site, no tiles, no LDS), bit for bit, spins and observables.

What this child adds
  * the start.  The quad table is indexed by the four counts of a count dword, i = c0 + 5 c1 + 25 c2 + 125 c3 (sites 0..3 or 4..7 of
    an octet, the 8 same-colour sites of 16 columns of a row).  Neighbouring sites of a dword share the spin between them, so a 4
    beside a 0 cannot occur: 13 neighbour spins decide the four counts, and enumerating their 8192 settings gives the index values
    that exist at all (REACHABLE, 479 of the 625).  A uniform random start meets the rare ones (all 13 spins alike: 2^-13 per
    dword) too seldom for small lattices, so the start is random with one all-up and one all-down block and, planted on every third
    row, one 3 x 9 patch of neighbour spins per reachable index value, cycling through them;
  * the condition.  The counts that the first half-sweep of a call takes are those of colour 0 ((row + column) even) in the state
    the call starts from.  The child tallies the index values of those dwords in the generic kernel's states at the start of every
    call (over the rows the tiled kernel owns) and fails a byte-plane periodic case that misses a reachable one;
  * "distinct", a table whose five degree-4 thresholds lie far apart and in no order;
  * renumber: a tile-resident handle at one sweep per generation, driven in calls of `call` sweeps until the strip numbering has
    restarted once (generation + call + 2 >= 16383), compared before and after the restart and one call later."""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))
import numpy as np  # noqa: E402
from tsu import _hip  # noqa: E402

GEN_LIMIT = 16383


def with_degree4(entries):
    """the critical temperature's table with its degree-4 row (the only one a periodic lattice reads) replaced"""
    t = _hip.ising2d_thresholds(1.0, 0.0, 2.269185).copy()
    t[20:25] = np.array(entries, dtype=np.uint64)
    return t


CLAMP = [0, 1 << 16, 0x7FFF8000, 0xFFFF0000, 1 << 32]
TABLES = {"tc": _hip.ising2d_thresholds(1.0, 0.0, 2.269185),
          "coarse": np.array([(k * 0x0A3D) << 16 | 0x8000 for k in range(25)], dtype=np.uint64),  # ties often: the tie path
          "field": _hip.ising2d_thresholds(1.0, 0.3, 2.0),
          "clamp_reversed": with_degree4(CLAMP[::-1]),
          # accept probabilities 0.10, 0.90, 0.30, 0.70, 0.50 for 0..4 up neighbours: a threshold taken from another position of
          # the entry, or an entry found with a wrong weight, differs from the right one by 0.2 of the range at least
          "distinct": with_degree4([int(p * 2 ** 32) for p in (0.10, 0.90, 0.30, 0.70, 0.50)])}


def neighbour_settings():
    """index value -> (h, u, d): the five spins between and beside the four sites of a dword (h[j], h[j + 1] are the horizontal
    neighbours of site j) and the four above / below them, 1 = up; the first setting found for every value that has one"""
    found = {}
    for bits in itertools.product((0, 1), repeat=13):
        h, u, d = bits[:5], bits[5:9], bits[9:]
        c = [h[j] + h[j + 1] + u[j] + d[j] for j in range(4)]
        found.setdefault(c[0] + 5 * c[1] + 25 * c[2] + 125 * c[3], (h, u, d))
    return found


SETTINGS = neighbour_settings()
REACHABLE = np.array(sorted(SETTINGS))
assert len(REACHABLE) == 479 and 0 in SETTINGS and 624 in SETTINGS and 4 not in SETTINGS  # (4, 0, 0, 0): a 4 beside a 0


def start_state(rows, cols, seed):
    """random spins, an all-up and an all-down block, and on rows 0, 3, 6, ... the low dword of every whole octet planted with the
    neighbour spins of one reachable index value after the other"""
    rng = np.random.default_rng(seed)
    up = rng.integers(0, 2, size=(rows, cols), dtype=np.int8)
    up[rows // 8:rows // 4, cols // 8:cols // 2] = 1
    up[rows // 2:rows // 2 + rows // 8, cols // 2:cols - cols // 8] = 0
    slot = 0
    for r in range(0, rows - 2, 3):
        for q in range(cols // 16):
            h, u, d = SETTINGS[int(REACHABLE[slot % len(REACHABLE)])]
            c0 = 16 * q + (r & 1)  # column of site 0 of colour 0 in this row
            for j in range(5):
                up[r, (c0 + 2 * j - 1) % cols] = h[j]
            for j in range(4):
                up[(r - 1) % rows, c0 + 2 * j] = u[j]
                up[(r + 1) % rows, c0 + 2 * j] = d[j]
            slot += 1
    return (2 * up - 1).astype(np.int8)


def dword_indices(spins, row_first, row_count):
    """index values of the colour-0 count dwords of rows [row_first, row_first + row_count) of a periodic lattice (whole octets)"""
    up = (spins > 0).astype(np.int64)
    cnt = np.roll(up, 1, 0) + np.roll(up, -1, 0) + np.roll(up, 1, 1) + np.roll(up, -1, 1)
    rows, cols = spins.shape
    noct = cols // 16
    out = []
    for r in range(row_first, row_first + row_count):
        c = cnt[r % rows, (r & 1):16 * noct:2].reshape(noct * 2, 4)  # four consecutive colour-0 sites = one dword
        out.append(c[:, 0] + 5 * c[:, 1] + 25 * c[:, 2] + 125 * c[:, 3])
    return np.concatenate(out)


def fail(case, what):
    print(f"MISMATCH {json.dumps(case)}: {what}")
    sys.exit(1)


def compare(case, lat, ref, slab, what):
    want = ref.get_spins()
    if slab:
        want = want[slab[0]:slab[0] + slab[1]]
    got = lat.get_spins()
    if not (got == want).all():
        bad = np.argwhere(got != want)
        fail(case, f"{what}: {len(bad)} sites differ, first {bad[:5].tolist()}")
    if not slab and lat.observables() != ref.observables():
        fail(case, f"{what}: observables")


def renumber(case, lat, ref):
    call, done = case["call"], 0
    restarts0 = None
    while True:
        g, r = lat.strip_numbering()
        due = done > 0 and g + call + 2 >= GEN_LIMIT
        if due:
            compare(case, lat, ref, None, f"before the restart at sweep {done}")
        l0 = lat.launch_count()
        lat.sweep(call, 13, done)
        ref.sweep(call, 13, done)
        done += call
        if lat.launch_count() - l0 != 1:
            fail(case, "not tile-resident")
        if restarts0 is None:
            restarts0 = lat.strip_numbering()[1]
        if due:
            if lat.strip_numbering() != (call, r + 1):
                fail(case, f"a restart was due at generation {g}: {lat.strip_numbering()}")
            compare(case, lat, ref, None, f"after the restart at sweep {done}")
            break
        if lat.strip_numbering() != (g + call, restarts0):
            fail(case, f"no restart was due at generation {g}: {lat.strip_numbering()}")
        if done > 2 * GEN_LIMIT:
            fail(case, "the numbering never restarted")
    lat.sweep(19, 13, done)
    ref.sweep(19, 13, done)
    compare(case, lat, ref, None, "one call after the restart")
    return done + 19


ctx = _hip.Context(0)
for index, case in enumerate(json.loads(sys.argv[1])):
    print(f"[case {index}]", file=sys.stderr, flush=True)  # the library's TSU_K1_VERBOSE lines of this case follow it on stderr
    rows, cols, k = case["rows"], case["cols"], case["k"]
    periodic = case.get("periodic", True)
    table = TABLES[case.get("table", "tc")]
    start = start_state(rows, cols, rows + cols)
    ref = _hip.Lattice(rows, cols, periodic, ctx=ctx)
    ref.set_kernel(_hip.KERNEL_GENERIC, 0)
    ref.set_spins(start)
    ref.set_thresholds(table)
    slab = case.get("slab")
    if slab:
        row0, own, ghost = slab
        lat = _hip.Lattice(own, cols, periodic, ctx=ctx, total_rows=rows, row0=row0, ghost=ghost)
    else:
        lat = _hip.Lattice(rows, cols, periodic, ctx=ctx)
        lat.set_spins(start)
    lat.set_kernel(_hip.KERNEL_TILED, k)
    lat.set_thresholds(table)
    if case.get("renumber"):
        total = renumber(case, lat, ref)
        print(f"ok {json.dumps(case)} sweeps={total}", flush=True)
        lat.close()
        ref.close()
        continue
    done, launches = 0, []
    seen = np.zeros(625, dtype=bool)
    for n in case["calls"]:
        full = ref.get_spins()
        if periodic:
            seen[dword_indices(full, slab[0] if slab else 0, slab[1] if slab else rows)] = True
        if slab:  # owned rows and ghost rows from the whole lattice (the window wraps on a periodic one)
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
        compare(case, lat, ref, slab, f"after {done} sweeps")
    if case.get("one_launch") and launches != [1] * len(case["calls"]):
        fail(case, f"not tile-resident: launches per call {launches}")
    missing = REACHABLE[~seen[REACHABLE]]
    if case.get("all_indices") and len(missing):
        fail(case, f"{len(missing)} reachable index values never occurred, first {missing[:8].tolist()}")
    if seen.sum() > len(REACHABLE):
        fail(case, "an index value occurred that no neighbour setting gives")
    print(f"ok {json.dumps(case)} launches={launches} indices={int(seen.sum())}", flush=True)
    lat.close()
    ref.close()
print("ALL OK")

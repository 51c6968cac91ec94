"""Child process of tests/test_far_end_gpu.py: TSU_TILE_VARIANT is read once per process, so a forced tile shape (the nibble planes
on a lattice small enough for the oracle) gets a process of its own.  argv[1] is a JSON object:

  {"mode": "sweeps", "rows", "cols", "periodic", "k", "seed", "replica", "calls": [[sweep0, n], ...]}
      the tiled kernel against the oracle, bit for bit, call after call; every call of more than k sweeps must be ONE launch
      (tile-resident)
  {"mode": "renumber", "rows", "cols", "periodic", "seed", "replica", "call", "restarts"}
      strip renumbering: a tile-resident handle with one sweep per generation runs calls of `call` sweeps until the strip numbering
      has restarted `restarts` times after its first start; the comparator is the same tile shape in the launch-per-generation form
      (calls of at most 8 sweeps at 8 sweeps per launch, which never go resident: tests/test_nibble_gpu.py pins that form to the
      oracle).  Spins and observables are compared before and after every call that restarts, and at the end.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))
import numpy as np  # noqa: E402
from oracle import oracle as ora  # noqa: E402
from tsu import _hip  # noqa: E402

GEN_LIMIT = 16383


def fail(msg):
    print("MISMATCH " + msg, flush=True)
    sys.exit(1)


def same(a, b, what):
    ga, gb = a.get_spins(), b.get_spins() if hasattr(b, "get_spins") else b
    if not (ga == gb).all():
        bad = np.argwhere(ga != gb)
        fail(f"{what}: {len(bad)} sites, first {bad[:5].tolist()}")
    return ga


def sweeps(ctx, c):
    rows, cols, periodic, k = c["rows"], c["cols"], bool(c["periodic"]), c["k"]
    seed, replica = c["seed"], c["replica"]
    table = ora.ising2d_thresholds(1.0, 0.05, 2.269185, 0)
    lat = _hip.Lattice(rows, cols, periodic, ctx=ctx)
    lat.set_kernel(_hip.KERNEL_TILED, k)
    lat.randomize(seed, replica)
    want = ora.ising2d_randomize(rows, cols, seed, replica)
    same(lat, want, "randomize")
    lat.set_thresholds(table)
    for sweep0, n in c["calls"]:
        n0 = lat.launch_count()
        lat.sweep(n, seed, sweep0, replica)
        launches = lat.launch_count() - n0
        want = ora.ising2d_sweep(want, periodic, table, n, seed, sweep0, replica)
        same(lat, want, f"{rows}x{cols} sweep0={sweep0} n={n}")
        if lat.observables() != ora.ising2d_observables(want, periodic):
            fail(f"observables after sweep0={sweep0}")
        if n > k and launches != 1:
            fail(f"{launches} launches for a call of {n} sweeps: not tile-resident")
        print(f"ok {rows}x{cols} sweep0={sweep0} n={n} launches={launches} numbering={lat.strip_numbering()}", flush=True)
    lat.close()


def renumber(ctx, c):
    rows, cols, periodic = c["rows"], c["cols"], bool(c["periodic"])
    seed, replica, call = c["seed"], c["replica"], c["call"]
    table = ora.ising2d_thresholds(1.0, 0.05, 2.269185, 0)
    res = _hip.Lattice(rows, cols, periodic, ctx=ctx)
    gen = _hip.Lattice(rows, cols, periodic, ctx=ctx)
    res.set_kernel(_hip.KERNEL_TILED, 1)
    gen.set_kernel(_hip.KERNEL_TILED, 8)
    for lat in (res, gen):
        lat.randomize(seed, replica)
        lat.set_thresholds(table)
    done, restarted, first = 0, 0, None
    while restarted < c["restarts"]:
        g, r = res.strip_numbering()
        due = first is not None and g + call + 2 >= GEN_LIMIT
        if due:
            same(res, gen, f"before the restart at sweep {done}")
        n0 = res.launch_count()
        res.sweep(call, seed, done, replica)
        if res.launch_count() - n0 != 1:
            fail("the resident handle did not make one launch per call")
        for s in range(0, call, 8):
            gen.sweep(min(8, call - s), seed, done + s, replica)
        done += call
        g1, r1 = res.strip_numbering()
        if first is None:
            first = r1
            if (g1, r1) != (call, 1):
                fail(f"numbering after the first call: {(g1, r1)}")
        elif due:
            if (g1, r1) != (call, r + 1):
                fail(f"a restart was due at generation {g} and the numbering reads {(g1, r1)}")
            restarted += 1
            same(res, gen, f"after the restart at sweep {done}")
            if res.observables() != gen.observables():
                fail(f"observables after the restart at sweep {done}")
        elif (g1, r1) != (g + call, r):
            fail(f"no restart was due at generation {g} and the numbering reads {(g1, r1)}")
        if done > 40 * GEN_LIMIT:
            fail("the numbering never restarted")
    same(res, gen, "at the end")
    if gen.strip_numbering() != (0, 0):
        fail(f"the comparator went tile-resident: {gen.strip_numbering()}")
    print(f"ok renumber {rows}x{cols} sweeps={done} restarts={restarted}", flush=True)
    res.close()
    gen.close()


if __name__ == "__main__":
    case = json.loads(sys.argv[1])
    context = _hip.Context(0)
    {"sweeps": sweeps, "renumber": renumber}[case["mode"]](context, case)
    print("ALL OK")

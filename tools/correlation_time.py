"""Correlation length: what the profile pass and the recording of the k_min modes cost (csrc/corr_dev.h).

    python tools/correlation_time.py pass 4096x4096 [--out DIR]        the profile pass of a pair against the overlap pass
    python tools/correlation_time.py round 256x256x256 --slots 8 [--out DIR]   a recorded ladder round with and without correlation

One process per shape.  `pass` times tsu_ising*_profiles(a, b) and tsu_ising*_overlap(a, b) of the same two random lattices in the
same run (device events around calls that end in a synchronise, both warmed up, medians of 9): both read 2 B per site, so the byte
count predicts a ratio near 1; the calls include their memset and their copy to the host (8 B for the overlap, 8 B per bin for the
profiles), which a kernel trace of the same command separates from the kernels.  `round` times rounds of `--sweeps` sweeps
of two ladders of `--slots` walkers, recorded, swaps on, with and without correlation (events around one run of several rounds,
medians of 5) and states the added cost as a share of the round.  Each call merges its rows into DIR/correlation_time.json and
rewrites DIR/correlation_time.txt from them (default DIR: profiles/)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))
from tsu import _hip  # noqa: E402
from tsu.models.ising import _kmin_tables  # noqa: E402


def median_ms(ctx, call, reps):
    call()
    ctx.synchronize()
    out = []
    for _ in range(reps):
        ctx.timer_begin()
        call()
        out.append(ctx.timer_end())
    return float(np.median(out))


def time_pass(shape):
    ctx = _hip.Context.default()
    cls = _hip.Lattice if len(shape) == 2 else _hip.Lattice3D
    a, b = cls(*shape, True, ctx=ctx), cls(*shape, True, ctx=ctx)
    try:
        a.randomize(3)
        b.randomize(4)
        q = a.overlap(b)
        assert all(int(p.sum()) == q for p in a.profiles(b)), "profiles do not sum to the overlap"
        ms_o = median_ms(ctx, lambda: a.overlap(b), 9)
        ms_p = median_ms(ctx, lambda: a.profiles(b), 9)
    finally:
        a.close()
        b.close()
    N = int(np.prod(shape))
    return dict(kind="pass", shape=list(shape), sites=N, overlap_ms=ms_o, profiles_ms=ms_p, ratio=ms_p / ms_o,
                overlap_bytes_per_s=2 * N / (ms_o * 1e-3), profiles_bytes_per_s=2 * N / (ms_p * 1e-3))


def time_round(shape, slots, sweeps, rounds):
    ctx = _hip.Context.default()
    rng = np.random.default_rng(1)
    cls = _hip.TemperingLattice if len(shape) == 2 else _hip.TemperingLattice3D
    dis = [rng.normal(size=shape).astype(np.float32) for _ in range(len(shape) + 1)]
    out = {}
    for corr in (False, True):
        pt = cls(*shape, True, slots, 2, ctx=ctx)
        try:
            pt.set_disorder(*dis[:-1], dis[-1])
            pt.set_temperatures(np.linspace(0.8, 2.4, slots))
            if corr:
                pt.set_correlation(True, [_kmin_tables(n) for n in shape])
            pt.init(5, 0)
            out[corr] = median_ms(ctx, lambda: pt.run(rounds, sweeps), 5) / rounds
        finally:
            pt.close()
    added = out[True] - out[False]
    N = int(np.prod(shape))
    return dict(kind="round", shape=list(shape), sites=N, slots=slots, ladders=2, sweeps_per_round=sweeps, rounds_per_run=rounds,
                round_ms=out[False], round_with_correlation_ms=out[True], added_ms=added, added_share=added / out[True],
                added_bytes_per_s=2 * N * slots / (added * 1e-3) if added > 0 else float("nan"))


def line(r):
    shape = "x".join(str(n) for n in r["shape"])
    if r["kind"] == "pass":
        return (f"pass  {shape:>12}: overlap {r['overlap_ms'] * 1e3:8.1f} us ({r['overlap_bytes_per_s'] / 1e12:.2f} TB/s)  "
                f"profiles {r['profiles_ms'] * 1e3:8.1f} us ({r['profiles_bytes_per_s'] / 1e12:.2f} TB/s on 2 B per site)  "
                f"profiles / overlap = {r['ratio']:.2f}")
    return (f"round {shape:>12} x {r['slots']:3d} slots x 2 ladders, {r['sweeps_per_round']:2d} sweeps/round: "
            f"{r['round_ms'] * 1e3:9.1f} us  with correlation {r['round_with_correlation_ms'] * 1e3:9.1f} us  "
            f"added {r['added_ms'] * 1e3:8.1f} us = {100 * r['added_share']:.1f} % of the round "
            f"({r['added_bytes_per_s'] / 1e12:.2f} TB/s on 2 B per site and slot)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("kind", choices=("pass", "round"))
    ap.add_argument("shape")
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    shape = tuple(int(n) for n in a.shape.split("x"))
    row = time_pass(shape) if a.kind == "pass" else time_round(shape, a.slots, a.sweeps, a.rounds)
    print(line(row), flush=True)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "correlation_time.json")
    doc = json.load(open(path)) if os.path.exists(path) else dict(rows=[])
    key = lambda r: (r["kind"], r["shape"], r.get("slots"), r.get("sweeps_per_round"))  # noqa: E731
    doc["rows"] = [r for r in doc["rows"] if key(r) != key(row)] + [row]
    doc["device"] = _hip.Context.default().device_info()
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(a.out, "correlation_time.txt"), "w") as f:
        f.write("\n".join(line(r) for r in doc["rows"]) + "\n")


if __name__ == "__main__":
    main()

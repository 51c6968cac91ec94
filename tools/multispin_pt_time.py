"""K9 tempering: time per round of MultispinTempering3D with and without the swap pass, against the plain glass's round (the
parent's figure, profiles/multispin_time.txt) and against the tempering ensemble with swaps on the same bimodal couplings,
measured in the same run.

Cases (periodic cubes, T ladder 0.5 ... 2.0, rounds of 10 sweeps), those of tools/multispin_time.py:
  16^3 x 32 T x 256 samples, one and two replicas   (small route)
   8^3 x 16 T x 1024 samples                        (small route)
  64^3 x  8 T x  64 samples                         (HBM route)
A round with swaps is the sweep launches plus k9_measure, k9_pt_plan and k9_pt_apply; run(swap=False, record=False) is the sweep
launches alone, which must cost what MultispinGlass3D.sweep costs.  The overhead is quoted as a fraction of that no-swap round.
The exchange's floor is 16 bytes per site-word and round (one read, one write) at the HBM peak of 8 TB/s.  Device events around
calls that end in a synchronise, every case warmed up, medians of 5, no profiler.

    python tools/multispin_pt_time.py [--out DIR] [--cases 16x32x256x1,16x32x256x2,8x16x1024x1,64x8x64x1] [--profile-case CASE]

Writes DIR/multispin_pt_time.txt (default DIR: profiles/).  --profile-case runs a few rounds of one case and nothing else, for a
kernel trace (rocprofv3 --kernel-trace --stats -- python tools/multispin_pt_time.py --profile-case 16x32x256x1)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))
from tsu import _hip  # noqa: E402
from tsu.models.ising import (LatticeTemperingEnsemble3D, MultispinGlass3D, MultispinTempering3D,  # noqa: E402
                              edwards_anderson_samples)

INTERVAL = 10
REPS = 5
HBM_PEAK = 8.0e12  # bytes/s


def temperatures(R):
    return np.linspace(0.5, 2.0, R)


def median_ms(run, rounds):
    ctx = _hip.Context.default()
    run(2)
    ctx.synchronize()
    out = []
    for _ in range(REPS):
        ctx.timer_begin()
        run(rounds)
        out.append(ctx.timer_end() / rounds)
    return float(np.median(out))


def time_plain(L, R, A, j, rounds):
    g = MultispinGlass3D(L, temperatures(R), couplings=j, replicas=A, seed=3)
    try:
        def run(n):
            for _ in range(n):
                g.sweep(INTERVAL)
        return median_ms(run, rounds), g.route
    finally:
        g.close()


def time_tempering(L, R, A, j, rounds):
    """(ms per round with swaps, ms per round without, mean acceptance), no record in either."""
    g = MultispinTempering3D(L, temperatures(R), couplings=j, replicas=A, seed=3)
    try:
        swap = median_ms(lambda n: g.run(n, INTERVAL, swap=True, record=False), rounds)
        none = median_ms(lambda n: g.run(n, INTERVAL, swap=False, record=False), rounds)
        acc = float(np.nanmean(g.acceptance()))
        return swap, none, acc
    finally:
        g.close()


def time_ensemble(L, R, A, j, rounds):
    pt = LatticeTemperingEnsemble3D(L, temperatures(R), couplings=j, seed=3, ladders=A)
    try:
        return median_ms(lambda n: pt.run(n, INTERVAL, swap=True, record=False), rounds)
    finally:
        pt.close()


def parse(case):
    return tuple(int(x) for x in case.split("x"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--cases", default="16x32x256x1,16x32x256x2,8x16x1024x1,64x8x64x1")
    ap.add_argument("--profile-case", default=None)
    a = ap.parse_args()
    ctx = _hip.Context.default()
    if a.profile_case:
        L, R, S, A = parse(a.profile_case)
        g = MultispinTempering3D(L, temperatures(R), couplings=edwards_anderson_samples(L, S, kind="bimodal", seed=1), replicas=A, seed=3)
        g.run(20, INTERVAL, record=False)
        ctx.synchronize()
        g.close()
        return
    lines = [f"device: {ctx.device_info()['name']}, {ctx.device_info()['compute_units']} CUs; rounds of {INTERVAL} sweeps, medians of {REPS}"]
    print(lines[0], flush=True)
    for case in a.cases.split(","):
        L, R, S, A = parse(case)
        j = edwards_anderson_samples(L, S, kind="bimodal", seed=1)
        updates = float(L) ** 3 * S * R * A * INTERVAL
        rounds = max(2, min(50, int(4e9 / updates)))
        plain, route = time_plain(L, R, A, j, rounds)
        swap, none, acc = time_tempering(L, R, A, j, rounds)
        ens = time_ensemble(L, R, A, j, rounds)
        words = float(L) ** 3 * ((S + 63) // 64) * R * A
        floor_us = 16.0 * words / HBM_PEAK * 1e6
        lines.append(f"{L}^3 x {R} T x {S} samples x {A} replica(s) ({route}): plain glass {plain * 1e3:8.1f} us/round | tempering, swap=False "
                     f"{none * 1e3:8.1f} | swap=True {swap * 1e3:8.1f} us/round = {updates / (swap * 1e-3):.3e} updates/s, overhead "
                     f"{(swap - none) * 1e3:6.1f} us = {100 * (swap - none) / none:5.1f} % of the no-swap round, mean acceptance {acc:.2f}")
        lines.append(f"    exchange floor (16 B x {words:.3g} site-words at 8 TB/s): {floor_us:6.2f} us | ensemble with swaps "
                     f"{ens * 1e3:9.1f} us/round, {ens / swap:.1f}x the multispin round")
        print(lines[-2], flush=True)
        print(lines[-1], flush=True)
        del j
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "multispin_pt_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

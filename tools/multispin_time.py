"""K9, multispin coding of the +-J glass: updates/s of MultispinGlass3D against the tempering ensemble (K8's k8_pte_sweep, one int8
per spin and one fp32 per bond) on the same bimodal couplings and temperatures, measured in the same run.

Cases (periodic cubes, T ladder 0.5 ... 2.0, rounds of 10 sweeps):
  16^3 x 32 T x 256 samples, one and two replicas   (small route: one launch per round)
   8^3 x 16 T x 1024 samples                        (small route)
  64^3 x  8 T x  64 samples                         (HBM route: one launch per half-sweep)
An update is one heat-bath decision of one spin of one sample: sites x samples x temperatures x replicas x sweeps.  The ensemble
runs LatticeTemperingEnsemble3D.run(swap=False) with ladders = replicas.  Device events around calls that end in a synchronise,
every case warmed up, medians of 5, no profiler.

    python tools/multispin_time.py [--out DIR] [--cases 16x32x256x1,16x32x256x2,8x16x1024x1,64x8x64x1]

Writes DIR/multispin_time.txt (default DIR: profiles/)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))
from tsu import _hip  # noqa: E402
from tsu.models.ising import LatticeTemperingEnsemble3D, MultispinGlass3D, edwards_anderson_samples  # noqa: E402

INTERVAL = 10
REPS = 5


def temperatures(R):
    return np.linspace(0.5, 2.0, R)


def time_multispin(L, R, S, A, j, rounds, route=None):
    """(median ms per round of INTERVAL sweeps, route, launches per round)."""
    ctx = _hip.Context.default()
    g = MultispinGlass3D(L, temperatures(R), couplings=j, replicas=A, seed=3, route=route)
    try:
        g.sweep(INTERVAL)
        ctx.synchronize()
        out = []
        n0 = g.launch_count
        for _ in range(REPS):
            ctx.timer_begin()
            for _ in range(rounds):
                g.sweep(INTERVAL)
            out.append(ctx.timer_end() / rounds)
        return float(np.median(out)), g.route, (g.launch_count - n0) / (REPS * rounds)
    finally:
        g.close()


def time_ensemble(L, R, A, j, rounds):
    """Median ms per round of INTERVAL sweeps of the tempering ensemble without swaps."""
    ctx = _hip.Context.default()
    pt = LatticeTemperingEnsemble3D(L, temperatures(R), couplings=j, seed=3, ladders=A)
    try:
        pt.run(2, INTERVAL, swap=False, record=False)
        ctx.synchronize()
        out = []
        for _ in range(REPS):
            ctx.timer_begin()
            pt.run(rounds, INTERVAL, swap=False, record=False)
            out.append(ctx.timer_end() / rounds)
        return float(np.median(out))
    finally:
        pt.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--cases", default="16x32x256x1,16x32x256x2,8x16x1024x1,64x8x64x1")
    a = ap.parse_args()
    ctx = _hip.Context.default()
    lines = [f"device: {ctx.device_info()['name']}, {ctx.device_info()['compute_units']} CUs; rounds of {INTERVAL} sweeps, medians of {REPS}"]
    print(lines[0], flush=True)
    for case in a.cases.split(","):
        L, R, S, A = (int(x) for x in case.split("x"))
        j = edwards_anderson_samples(L, S, kind="bimodal", seed=1)
        updates = float(L) ** 3 * S * R * A * INTERVAL
        rounds = max(2, min(50, int(4e9 / updates)))
        ms, route, launches = time_multispin(L, R, S, A, j, rounds)
        ms_ens = time_ensemble(L, R, A, j, rounds)
        ups, ups_ens = updates / (ms * 1e-3), updates / (ms_ens * 1e-3)
        lines.append(f"{L}^3 x {R} T x {S} samples x {A} replica(s): multispin ({route}, {launches:.0f} launch(es)/round) {ms * 1e3:10.1f} us/round "
                     f"{ups:.3e} updates/s | ensemble {ms_ens * 1e3:10.1f} us/round {ups_ens:.3e} walker-updates/s | ratio {ups / ups_ens:.2f}x")
        print(lines[-1], flush=True)
        if route == "small":  # the same planes through the HBM route, for the record
            ms_h, _, launches_h = time_multispin(L, R, S, A, j, rounds, route="hbm")
            lines.append(f"    the same on the hbm route ({launches_h:.0f} launches/round): {ms_h * 1e3:10.1f} us/round "
                         f"{updates / (ms_h * 1e-3):.3e} updates/s | ratio {ms_ens / ms_h:.2f}x")
            print(lines[-1], flush=True)
        del j
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "multispin_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

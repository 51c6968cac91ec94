"""K9 correlation record: time per recorded round of MultispinTempering3D with a swap pass, correlation off and on in the same run.

Cases (periodic cubes, T ladder 0.5 ... 2.0, rounds of 10 sweeps), those of tools/multispin_pt_time.py:
  16^3 x 32 T x 256 samples, one and two replicas   (small route)
   8^3 x 16 T x 1024 samples                        (small route)
  64^3 x  8 T x  64 samples                         (HBM route)
A recorded round with swaps is the sweep launches plus k9_measure, k9_pt_plan and k9_pt_apply; with correlation=True it also takes
k9_profile and k9_modes between the measurement and the pass.  The added time is quoted absolutely and as a fraction of the
correlation-off round of the same run; k9_measure's own time comes from a kernel trace of one case, collected in a run of its
own (--profile-case).  Device events around calls that end in a synchronise, every case warmed up, medians of 5, no profiler.

    python tools/multispin_corr_time.py [--out DIR] [--cases 16x32x256x1,16x32x256x2,8x16x1024x1,64x8x64x1] [--profile-case CASE]

Writes DIR/multispin_corr_time.txt (default DIR: profiles/).  --profile-case runs a few recorded rounds of one case with
correlation on and nothing else, for a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/multispin_corr_time.py --profile-case 16x32x256x2)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))
from tsu import _hip  # noqa: E402
from tsu.models.ising import MultispinTempering3D, edwards_anderson_samples  # noqa: E402

INTERVAL = 10
REPS = 5


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


def time_recorded(L, R, A, j, rounds, correlation):
    """ms per recorded round with swaps; the record stays on the device (the handle's run, not the class's, which fetches it)."""
    g = MultispinTempering3D(L, temperatures(R), couplings=j, replicas=A, seed=3, correlation=correlation)
    state = {"sweep": 0, "round": 0}

    def run(n):
        g._msc.pt_run(n, INTERVAL, True, True, state["sweep"], state["round"])
        state["sweep"] += n * INTERVAL
        state["round"] += n

    try:
        return median_ms(run, rounds), g.route
    finally:
        g.close()


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
        g = MultispinTempering3D(L, temperatures(R), couplings=edwards_anderson_samples(L, S, kind="bimodal", seed=1), replicas=A, seed=3,
                                 correlation=True)
        g._msc.pt_run(20, INTERVAL, True, True, 0, 0)
        ctx.synchronize()
        g.close()
        return
    lines = [f"device: {ctx.device_info()['name']}, {ctx.device_info()['compute_units']} CUs; recorded rounds of {INTERVAL} sweeps with a "
             f"swap pass, medians of {REPS}"]
    print(lines[0], flush=True)
    for case in a.cases.split(","):
        L, R, S, A = parse(case)
        j = edwards_anderson_samples(L, S, kind="bimodal", seed=1)
        updates = float(L) ** 3 * S * R * A * INTERVAL
        rounds = max(2, min(50, int(4e9 / updates)))
        off, route = time_recorded(L, R, A, j, rounds, False)
        on, _ = time_recorded(L, R, A, j, rounds, True)
        lines.append(f"{L}^3 x {R} T x {S} samples x {A} replica(s) ({route}): correlation off {off * 1e3:8.1f} us/round | on "
                     f"{on * 1e3:8.1f} us/round | added {(on - off) * 1e3:6.1f} us = {100 * (on - off) / off:5.1f} % of the correlation-off round")
        print(lines[-1], flush=True)
        del j
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "multispin_corr_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""K9 quench records: the time of one C4 row, one two-time row and one snapshot beside a round of 10 sweeps, in the same run.

Cases (periodic cubes, T ladder 0.5 ... 2.0, two replicas), those of tools/multispin_pt_time.py:
  16^3 x 32 T x 256 samples   (small route)
  64^3 x  8 T x  64 samples   (HBM route)
Everything runs on one MultispinTempering3D handle per case, swaps off, and every figure is a time per round of 10 sweeps:
  sweeps      tsu_msc_sweep(10) alone
  measured    tsu_msc_pt_run, recording, no swap pass: the sweeps and k9_measure
  quench      tsu_msc_quench_run with times 10 apart: the sweeps, k9_measure and one C4 row (a memset and k9_c4)
  quench + tw the same with one waiting time at the first row: one two-time row (k9_twotime) more per row
so a C4 row is quench - measured and a two-time row is (quench + tw) - quench; a snapshot is timed on its own (device-to-device
copies of all planes in a row).  Device events around calls that end in a synchronise, every case warmed up, medians of 5, no
profiler.

    python tools/multispin_quench_time.py [--out DIR] [--cases 16x32x256,64x8x64] [--profile-case CASE]

Writes DIR/multispin_quench_time.txt (default DIR: profiles/).  --profile-case runs one quench of 20 rows with one waiting time of
one case and nothing else, for a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/multispin_quench_time.py --profile-case 16x32x256)."""
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
ROWS = 20


def temperatures(R):
    return np.linspace(0.5, 2.0, R)


def median_ms(run, per_call):
    ctx = _hip.Context.default()
    run()
    ctx.synchronize()
    out = []
    for _ in range(REPS):
        ctx.timer_begin()
        run()
        out.append(ctx.timer_end() / per_call)
    return float(np.median(out))


def parse(case):
    return tuple(int(x) for x in case.split("x"))


def handle(L, R, S):
    g = MultispinTempering3D(L, temperatures(R), couplings=edwards_anderson_samples(L, S, kind="bimodal", seed=1), replicas=2, seed=3)
    g._msc.snapshot_slots(1)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--cases", default="16x32x256,64x8x64")
    ap.add_argument("--profile-case", default=None)
    a = ap.parse_args()
    ctx = _hip.Context.default()
    times = np.arange(1, ROWS + 1) * INTERVAL
    if a.profile_case:
        g = handle(*parse(a.profile_case))
        g._msc.quench_run(times, 0, [0])
        ctx.synchronize()
        g.close()
        return
    lines = [f"device: {ctx.device_info()['name']}, {ctx.device_info()['compute_units']} CUs; two replicas, rounds of {INTERVAL} sweeps, "
             f"{ROWS} rounds per call, medians of {REPS}"]
    print(lines[0], flush=True)
    for case in a.cases.split(","):
        L, R, S = parse(case)
        g = handle(L, R, S)
        m = g._msc
        state = {"sweep": 0, "round": 0}

        def sweeps():
            for _ in range(ROWS):
                m.sweep(INTERVAL, state["sweep"])
                state["sweep"] += INTERVAL

        def measured():
            m.pt_run(ROWS, INTERVAL, False, True, state["sweep"], state["round"])
            state["sweep"] += ROWS * INTERVAL
            state["round"] += ROWS

        def quench(waits=()):
            m.quench_run(times, state["sweep"], waits)
            state["sweep"] += ROWS * INTERVAL

        def snapshots():
            for _ in range(ROWS):
                m.snapshot(0)

        try:
            t_sweep = median_ms(sweeps, ROWS)
            t_meas = median_ms(measured, ROWS)
            t_q = median_ms(quench, ROWS)
            t_qw = median_ms(lambda: quench([0]), ROWS)
            t_snap = median_ms(snapshots, ROWS)
            route = g.route
        finally:
            g.close()
        c4, tt = t_q - t_meas, t_qw - t_q
        lines.append(f"{L}^3 x {R} T x {S} samples x 2 replicas ({route}), us per round: sweeps {t_sweep * 1e3:8.1f} | measured "
                     f"{t_meas * 1e3:8.1f} | quench {t_q * 1e3:8.1f} | quench + tw {t_qw * 1e3:8.1f}")
        lines.append(f"    one C4 row {c4 * 1e3:8.1f} us = {c4 / t_sweep:5.2f} of the {INTERVAL} sweeps | one two-time row {tt * 1e3:7.1f} us = "
                     f"{tt / t_sweep:5.3f} | one snapshot {t_snap * 1e3:7.1f} us = {t_snap / t_sweep:5.3f}")
        print("\n".join(lines[-2:]), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "multispin_quench_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""K7 parallel tempering: walker-updates/s and us per round of LatticeTempering (Gaussian J + h, T ladder 0.5 ... 2.0,
swap_interval 10) at 64^2 x 32, 256^2 x 32, 1024^2 x 16 and 4096^2 x 16 walkers, against the per-walker route
(IsingModel2D.gibbs_update per temperature + energy() per walker per round), with the bytes a batched sweep moves and the fraction
of the HBM and VALU-issue ceilings reached.  At 4096^2 the batched sweep is also timed with TSU_PT_GROUP = 1, 4 and 16.

    python tools/tempering_time.py [--out DIR] [--cases 64x32,256x32,1024x16,4096x16] [--rounds N]

Writes DIR/tempering_time.txt and DIR/tempering_time.json (default DIR: profiles/)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))
from tsu import _hip  # noqa: E402
from tsu.models.ising import IsingModel2D, LatticeTempering  # noqa: E402

HBM_PEAK = 8.0e12      # bytes/s, MI355X nominal
ISSUE_CEIL = 8.0e11    # updates/s: ~45 lane-instructions per site on the screened path
INTERVAL = 10


def disorder(L, seed=1):
    rng = np.random.default_rng(seed)
    return tuple(rng.normal(size=(L, L)).astype(np.float32) for _ in range(3))


def bytes_per_walker_sweep(L, W):
    """Spins (read C, U, D rows mostly from L2 and write C: ~4 B per site) + the 24 B per site of disorder shared by W walkers."""
    return L * L * (4.0 + 24.0 / W)


def group_of(L, nw, cus):
    """The walker-group size pt_group (csrc/pt_host.h, the one both ladder types call) picks."""
    lanes = L * ((L + 15) // 16)
    groups = -(-cus * 1024 // lanes)
    return 1 if groups >= nw else -(-nw // groups)


def time_batched(L, R, rounds, swap=True):
    jr, jd, h = disorder(L)
    ctx = _hip.Context.default()
    pt = LatticeTempering(L, np.linspace(0.5, 2.0, R), couplings=(jr, jd), field=h, seed=3)
    try:
        pt.run(2, INTERVAL, swap=swap, record=False)
        ctx.synchronize()
        ctx.timer_begin()
        pt.run(rounds, INTERVAL, swap=swap, record=False)
        return ctx.timer_end() / rounds
    finally:
        pt._pt.close()


def time_per_walker(L, R, rounds):
    jr, jd, h = disorder(L)
    models = [IsingModel2D(L, temperature=float(T), seed=3 + i, couplings=(jr, jd), field=h)
              for i, T in enumerate(np.linspace(0.5, 2.0, R))]
    try:
        for m in models:
            m.gibbs_update(INTERVAL)
            m.energy()
        t0 = time.perf_counter()
        for _ in range(rounds):
            for m in models:
                m.gibbs_update(INTERVAL)
            for m in models:
                m.energy()  # synchronises: one host round trip per walker
        return (time.perf_counter() - t0) * 1e3 / rounds
    finally:
        for m in models:
            m._lat.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--cases", default="64x32,256x32,1024x16,4096x16")
    ap.add_argument("--rounds", type=int, default=0, help="rounds per timing (default: by size)")
    a = ap.parse_args()
    ctx = _hip.Context.default()
    cus = ctx.device_info()["compute_units"]
    rows, lines = [], []
    for case in a.cases.split(","):
        L, R = (int(x) for x in case.split("x"))
        rounds = a.rounds or max(3, min(200, int(2e9 / (L * L * R * INTERVAL))))
        W = group_of(L, R, cus)
        ms_round = time_batched(L, R, rounds)
        ms_sweeps = time_batched(L, R, rounds, swap=False)
        ms_walker = time_per_walker(L, R, max(2, rounds // 4))
        ups = L * L * R * INTERVAL / (ms_sweeps * 1e-3)
        bw = bytes_per_walker_sweep(L, W) * R * INTERVAL / (ms_sweeps * 1e-3)
        row = dict(L=L, walkers=R, group=W, rounds=rounds, us_per_round=ms_round * 1e3, us_per_round_sweeps_only=ms_sweeps * 1e3,
                   us_per_round_per_walker_route=ms_walker * 1e3, walker_updates_per_s=ups,
                   walker_updates_per_s_with_swaps=L * L * R * INTERVAL / (ms_round * 1e-3),
                   per_walker_route_updates_per_s=L * L * R * INTERVAL / (ms_walker * 1e-3), bytes_per_s=bw,
                   hbm_fraction=bw / HBM_PEAK, issue_fraction=ups / ISSUE_CEIL)
        rows.append(row)
        lines.append(f"{L}^2 x {R} walkers (W = {W}): {ms_round * 1e3:10.1f} us/round with swaps ({ms_sweeps * 1e3:.1f} sweeps only)  "
                     f"{ups:.3e} walker-updates/s  per-walker route {ms_walker * 1e3:10.1f} us/round "
                     f"({row['per_walker_route_updates_per_s']:.3e})  speed-up {ms_walker / ms_round:.2f}x  "
                     f"{bw / 1e12:.2f} TB/s = {bw / HBM_PEAK:.2f} of HBM peak, {ups / ISSUE_CEIL:.2f} of the issue ceiling")
        print(lines[-1], flush=True)
    if any(c.startswith("4096x") for c in a.cases.split(",")):
        for g in (1, 4, 16):
            os.environ["TSU_PT_GROUP"] = str(g)
            ms = time_batched(4096, 16, 5, swap=False)
            ups = 4096 * 4096 * 16 * INTERVAL / (ms * 1e-3)
            bw = bytes_per_walker_sweep(4096, g) * 16 * INTERVAL / (ms * 1e-3)
            rows.append(dict(L=4096, walkers=16, group=g, forced=True, us_per_round_sweeps_only=ms * 1e3, walker_updates_per_s=ups,
                             bytes_per_s=bw, hbm_fraction=bw / HBM_PEAK, issue_fraction=ups / ISSUE_CEIL))
            lines.append(f"4096^2 x 16, TSU_PT_GROUP={g:2d}: {ms * 1e3:10.1f} us per 10 sweeps of all walkers  {ups:.3e} walker-updates/s  "
                         f"{bw / 1e12:.2f} TB/s = {bw / HBM_PEAK:.2f} of HBM peak, {ups / ISSUE_CEIL:.2f} of the issue ceiling")
            print(lines[-1], flush=True)
        os.environ.pop("TSU_PT_GROUP", None)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "tempering_time.json"), "w") as f:
        json.dump(dict(interval=INTERVAL, hbm_peak=HBM_PEAK, issue_ceiling=ISSUE_CEIL, device=ctx.device_info(), rows=rows), f, indent=1)
    with open(os.path.join(a.out, "tempering_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

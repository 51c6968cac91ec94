"""K8 parallel tempering: us per round and walker-updates/s of LatticeTempering3D (periodic cubes, Gaussian J + h, T ladder
0.5 ... 2.0, swap_interval 10) at 16^3 x 32, 64^3 x 32, 128^3 x 16 and 256^3 x 8 walkers.  In the same run, on code the ladders
do not touch: the walker-by-walker route (IsingModel3D.gibbs_update per temperature + energy() per walker per round) and
k8_sweep's single-lattice rate.  Device events around calls that end in a synchronise, every shape warmed up, medians of 5.
Bytes are counted on the model 4 + 32 / W B per walker-site and sweep (W = walkers per lane).  At 256^3 x 8 the batched sweep is
also timed with TSU_PT_GROUP = 1, 2 and 8.

Acceptance (exit status 1 if missed): per walker-update the batched sweep is more than 1.1x faster than k8_sweep alone at
256^3 x 8, and a batched round (sweeps, energies, swap pass) is more than 1.1x faster than a round of the walker-by-walker route
at 64^3 x 32.

    python tools/tempering3d_time.py [--out DIR] [--cases 16x32,64x32,128x16,256x8]

Writes DIR/tempering3d_time.txt and DIR/tempering3d_time.json (default DIR: profiles/)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))
from tsu import _hip  # noqa: E402
from tsu.models.ising import IsingModel3D, LatticeTempering3D  # noqa: E402

HBM_PEAK = 8.0e12      # bytes/s, MI355X nominal
INTERVAL = 10
MARGIN = 1.1
REPS = 5


def disorder(L, seed=1):
    rng = np.random.default_rng(seed)
    return tuple(rng.normal(size=(L, L, L)).astype(np.float32) for _ in range(4))


def temperatures(R):
    return np.linspace(0.5, 2.0, R)


def bytes_per_walker_sweep(L, W):
    """Spins (read the own row and four neighbour rows mostly from L2, write the own row: ~4 B per site and sweep) + the 32 B per
    site of disorder a sweep reads, shared by the W walkers of a lane."""
    return L ** 3 * (4.0 + 32.0 / W)


def group_of(L, nw, cus):
    """The walker-group size pt_group (csrc/pt_host.h, the one both ladder types call) picks."""
    lanes = L * L * ((L + 15) // 16)
    groups = -(-cus * 1024 // lanes)
    return 1 if groups >= nw else -(-nw // groups)


def rounds_for(L, R):
    return max(2, min(50, int(2e9 / (L ** 3 * R * INTERVAL))))


def time_batched(L, R, dis, rounds, swap=True):
    """Median ms per round of `rounds` rounds per call."""
    ctx = _hip.Context.default()
    pt = LatticeTempering3D(L, temperatures(R), couplings=dis[:3], field=dis[3], seed=3)
    try:
        pt.run(2, INTERVAL, swap=swap, record=False)
        ctx.synchronize()
        out = []
        for _ in range(REPS):
            ctx.timer_begin()
            pt.run(rounds, INTERVAL, swap=swap, record=False)
            out.append(ctx.timer_end() / rounds)
        return float(np.median(out))
    finally:
        pt._pt.close()


def time_per_walker(L, R, dis, rounds):
    """Median ms per round of the route without the ladders: one IsingModel3D per temperature, swept and read one by one."""
    models = [IsingModel3D(L, temperature=float(T), seed=3 + i, couplings=dis[:3], field=dis[3]) for i, T in enumerate(temperatures(R))]
    try:
        for m in models:
            m.gibbs_update(INTERVAL)
            m.energy()
        out = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            for _ in range(rounds):
                for m in models:
                    m.gibbs_update(INTERVAL)
                for m in models:
                    m.energy()  # synchronises: one host round trip per walker
            out.append((time.perf_counter() - t0) * 1e3 / rounds)
        return float(np.median(out))
    finally:
        for m in models:
            m._lat.close()


def time_k8(L, dis, per_call):
    """Median ms per sweep of k8_sweep on one lattice (tsu_ising3d_sweep), `per_call` sweeps per call."""
    ctx = _hip.Context.default()
    lat = _hip.Lattice3D(L, L, L, True, ctx=ctx)
    try:
        lat.randomize(3)
        lat.set_disorder(*dis)
        lat.sweep(1.0, 2, 7, 0)
        ctx.synchronize()
        out, sw = [], 2
        for _ in range(REPS):
            ctx.timer_begin()
            lat.sweep(1.0, per_call, 7, sw)
            out.append(ctx.timer_end() / per_call)
            sw += per_call
        return float(np.median(out))
    finally:
        lat.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--cases", default="16x32,64x32,128x16,256x8")
    a = ap.parse_args()
    ctx = _hip.Context.default()
    cus = ctx.device_info()["compute_units"]
    rows, lines, verdicts = [], [], []
    os.environ.pop("TSU_PT_GROUP", None)
    for case in a.cases.split(","):
        L, R = (int(x) for x in case.split("x"))
        dis = disorder(L)
        rounds = rounds_for(L, R)
        W = group_of(L, R, cus)
        updates = L ** 3 * R * INTERVAL
        ms_round = time_batched(L, R, dis, rounds)
        ms_sweeps = time_batched(L, R, dis, rounds, swap=False)
        ms_walker = time_per_walker(L, R, dis, max(2, rounds // 4))
        ms_k8 = time_k8(L, dis, INTERVAL * max(1, rounds // 2))
        ups = updates / (ms_sweeps * 1e-3)
        k8_ups = L ** 3 / (ms_k8 * 1e-3)
        bw = bytes_per_walker_sweep(L, W) * R * INTERVAL / (ms_sweeps * 1e-3)
        row = dict(L=L, walkers=R, group=W, rounds=rounds, us_per_round=ms_round * 1e3, us_per_round_sweeps_only=ms_sweeps * 1e3,
                   energy_and_swap_share=1.0 - ms_sweeps / ms_round, us_per_round_walker_by_walker=ms_walker * 1e3,
                   walker_updates_per_s=ups, walker_updates_per_s_with_swaps=updates / (ms_round * 1e-3),
                   walker_by_walker_updates_per_s=updates / (ms_walker * 1e-3), k8_sweep_us_per_sweep=ms_k8 * 1e3,
                   k8_sweep_updates_per_s=k8_ups, bytes_per_s=bw, hbm_fraction=bw / HBM_PEAK,
                   sweep_speedup_over_k8_sweep=ups / k8_ups, round_speedup_over_walker_by_walker=ms_walker / ms_round,
                   sweep_speedup_over_walker_by_walker=ms_walker / ms_sweeps)
        rows.append(row)
        lines.append(f"{L}^3 x {R} walkers (W = {W}): {ms_round * 1e3:10.1f} us/round with energies and swaps ({ms_sweeps * 1e3:.1f} sweeps "
                     f"only, energy + swap share {row['energy_and_swap_share']:.3f})  {ups:.3e} walker-updates/s  "
                     f"{bw / 1e12:.2f} TB/s = {bw / HBM_PEAK:.2f} of HBM peak | walker by walker {ms_walker * 1e3:10.1f} us/round "
                     f"({row['walker_by_walker_updates_per_s']:.3e}): round {ms_walker / ms_round:.2f}x, sweeps {ms_walker / ms_sweeps:.2f}x | "
                     f"k8_sweep alone {ms_k8 * 1e3:.1f} us/sweep ({k8_ups:.3e}): {ups / k8_ups:.2f}x per walker-update")
        print(lines[-1], flush=True)
        if (L, R) == (256, 8):
            verdicts.append(("batched sweep over k8_sweep alone at 256^3 x 8", ups / k8_ups))
            for g in (1, 2, 8):
                os.environ["TSU_PT_GROUP"] = str(g)
                ms = time_batched(L, R, dis, rounds, swap=False)
                os.environ.pop("TSU_PT_GROUP", None)
                g_ups = updates / (ms * 1e-3)
                g_bw = bytes_per_walker_sweep(L, g) * R * INTERVAL / (ms * 1e-3)
                rows.append(dict(L=L, walkers=R, group=g, forced=True, us_per_round_sweeps_only=ms * 1e3, walker_updates_per_s=g_ups,
                                 bytes_per_s=g_bw, hbm_fraction=g_bw / HBM_PEAK, sweep_speedup_over_k8_sweep=g_ups / k8_ups))
                lines.append(f"{L}^3 x {R}, TSU_PT_GROUP={g}: {ms * 1e3:10.1f} us per {INTERVAL} sweeps of all walkers  {g_ups:.3e} "
                             f"walker-updates/s  {g_bw / 1e12:.2f} TB/s = {g_bw / HBM_PEAK:.2f} of HBM peak  {g_ups / k8_ups:.2f}x k8_sweep")
                print(lines[-1], flush=True)
        if (L, R) == (64, 32):
            # like with like: the route's round holds its energies, so the batched round holds them (and the swap pass) too
            verdicts.append(("batched round over the walker-by-walker route at 64^3 x 32", ms_walker / ms_round))
        del dis
    ok = True
    for what, ratio in verdicts:
        passed = ratio > MARGIN
        ok = ok and passed
        lines.append(f"acceptance: {what}: {ratio:.2f}x (needs > {MARGIN}x): {'met' if passed else 'MISSED'}")
        print(lines[-1], flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "tempering3d_time.json"), "w") as f:
        json.dump(dict(interval=INTERVAL, hbm_peak=HBM_PEAK, margin=MARGIN, device=ctx.device_info(), rows=rows,
                       acceptance=[dict(what=w, ratio=r, met=bool(r > MARGIN)) for w, r in verdicts]), f, indent=1)
    with open(os.path.join(a.out, "tempering3d_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()

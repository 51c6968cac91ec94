"""Population annealing: the time of a step and of its parts (PopulationAnnealing / PopulationAnnealing3D, periodic lattices, Gaussian
J, theta = 10 sweeps per step) at 64^2 x 4096, 64^2 x 65535, 16^3 x 8192 and 4096^2 x 64 walkers.  Device events around calls that
end in a synchronise, every shape warmed up, medians of 3.  Per shape:

  step            a resampling step: plan, copy, theta sweeps, one energy pass (run(resample=True, record=False))
  plain step      the same without plan and copy (run(resample=False)); the difference is what resampling costs
  energy pass     tsu_pa*_energies (with its copy of R energies to the host)
  sweeps          plain step - energy pass, and the walker-updates/s that makes
  plan            the resampling cost on a schedule of db = 1e-12, where nobody dies and the copy has nothing to do
  copy            the resampling cost on the working schedule minus the plan; bytes = 2 x plane x the walkers that died (from a
                  recorded run of the same schedule), against HBM peak
  ladder          LatticeTempering / LatticeTempering3D with 256 walkers on the same lattice and disorder, swap=False, record=False:
                  the same sweep kernel, walker-updates/s in the same session

The working schedule steps by db = 0.5 / sqrt(dim N) from beta = 0.5, about half the high-temperature spread of E in the exponent.

    python tools/population_time.py [--out DIR] [--cases 2d:64x4096,2d:64x65535,3d:16x8192,2d:4096x64]

Writes DIR/population_time.txt and DIR/population_time.json (default DIR: profiles/)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))
from tsu import _hip  # noqa: E402
from tsu.models import ising  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X nominal
THETA = 10
REPS = 3


def median_ms(ctx, call, per):
    out = []
    for _ in range(REPS):
        ctx.timer_begin()
        call()
        out.append(ctx.timer_end() / per)
    return float(np.median(out))


def population(dim, L, R, dis, betas):
    cls = ising.PopulationAnnealing if dim == 2 else ising.PopulationAnnealing3D
    return cls((L,) * dim, R, betas=betas, couplings=dis, seed=3, sweeps_per_step=THETA)


def time_steps(ctx, dim, L, R, dis, betas, n, resample):
    """Median ms per step of n steps per call."""
    pa = population(dim, L, R, dis, betas)
    try:
        pa.run(n, resample=resample, record=False)
        ctx.synchronize()
        return median_ms(ctx, lambda: pa.run(n, resample=resample, record=False), n)
    finally:
        pa._pa.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--cases", default="2d:64x4096,2d:64x65535,3d:16x8192,2d:4096x64")
    a = ap.parse_args()
    ctx = _hip.Context.default()
    os.environ.pop("TSU_PT_GROUP", None)
    rows, lines = [], []
    for case in a.cases.split(","):
        d, rest = case.split(":")
        dim = int(d[0])
        L, R = (int(x) for x in rest.split("x"))
        N = L ** dim
        rng = np.random.default_rng(1)
        dis = tuple(rng.normal(size=(L,) * dim).astype(np.float32) for _ in range(dim))
        n = max(1, min(8, int(4e9 / (N * R * THETA))))
        K = (REPS + 1) * n
        db = 0.5 / np.sqrt(dim * N)
        work = 0.5 + db * np.arange(K + 1)
        still = 0.5 + 1e-12 * np.arange(K + 1)
        ms_step = time_steps(ctx, dim, L, R, dis, work, n, True)
        ms_plain = time_steps(ctx, dim, L, R, dis, work, n, False)
        ms_still = time_steps(ctx, dim, L, R, dis, still, n, True)
        pa = population(dim, L, R, dis, work)
        try:
            h = pa.run(K)
            died = float((h["parent"] != np.arange(R)).mean())
            pitch = (L + 255) // 256 * 256 if dim == 2 else (L + 15) // 16 * 16
            plane = L ** (dim - 1) * pitch
            ms_energy = median_ms(ctx, pa.energies, 1)
        finally:
            pa._pa.close()
        lt_cls = ising.LatticeTempering if dim == 2 else ising.LatticeTempering3D
        pt = lt_cls((L,) * dim, np.linspace(2.0, 1.0, 256), couplings=dis, seed=3)
        try:
            rounds = max(1, min(8, int(4e9 / (N * 256 * THETA))))
            pt.run(rounds, THETA, swap=False, record=False)
            ctx.synchronize()
            ms_ladder = median_ms(ctx, lambda: pt.run(rounds, THETA, swap=False, record=False), rounds)
        finally:
            pt._pt.close()
        ms_sweeps = ms_plain - ms_energy
        ms_plan = ms_still - ms_plain
        ms_resample = ms_step - ms_plain
        ms_copy = ms_resample - ms_plan
        copy_bytes = 2.0 * plane * died * R
        ups = N * R * THETA / (ms_sweeps * 1e-3)
        ladder_ups = N * 256 * THETA / (ms_ladder * 1e-3)
        row = dict(dim=dim, L=L, population=R, steps_per_call=n, db=db, died_per_step=died, us_step=ms_step * 1e3,
                   us_plain_step=ms_plain * 1e3, us_energy=ms_energy * 1e3, us_sweeps=ms_sweeps * 1e3, us_plan=ms_plan * 1e3,
                   us_copy=ms_copy * 1e3, resampling_share=ms_resample / ms_step, copy_bytes_per_step=copy_bytes,
                   copy_bytes_per_s=copy_bytes / (ms_copy * 1e-3) if ms_copy > 0 else float("nan"), walker_updates_per_s=ups,
                   ladder_256_walker_updates_per_s=ladder_ups, population_over_ladder=ups / ladder_ups)
        rows.append(row)
        lines.append(f"{L}^{dim} x {R} walkers, theta = {THETA}: step {ms_step * 1e3:10.1f} us = sweeps {ms_sweeps * 1e3:.1f} + energy pass "
                     f"{ms_energy * 1e3:.1f} + plan {ms_plan * 1e3:.1f} + copy {ms_copy * 1e3:.1f} (resampling {ms_resample / ms_step:.3f} of the "
                     f"step; {died:.3f} of the walkers die per step: {copy_bytes / 1e6:.1f} MB at {row['copy_bytes_per_s'] / 1e12:.2f} TB/s = "
                     f"{row['copy_bytes_per_s'] / HBM_PEAK:.2f} of HBM peak) | sweeps {ups:.3e} walker-updates/s, ladder of 256 walkers "
                     f"{ladder_ups:.3e}: {ups / ladder_ups:.2f}x")
        print(lines[-1], flush=True)
        del dis
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "population_time.json"), "w") as f:
        json.dump(dict(theta=THETA, hbm_peak=HBM_PEAK, device=ctx.device_info(), rows=rows), f, indent=1)
    with open(os.path.join(a.out, "population_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

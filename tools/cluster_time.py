"""K6 Swendsen-Wang: ms per step by lattice size and temperature (device events after warm-up), the step's byte floor and the
fraction of it reached, and the integrated autocorrelation time of |m| at T_c under SW against heat-bath sweeps.

    python tools/cluster_time.py [--out DIR] [--steps-only] [--sizes 1024,4096,...]

--steps-only skips the autocorrelation part (the command a rocprofv3 --kernel-trace --stats run profiles).  Writes
DIR/cluster_time.txt and DIR/cluster_time.json (default DIR: profiles/)."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))
from tsu import _hip  # noqa: E402
from tsu.models.ising import IsingModel2D  # noqa: E402

TC = 2.0 / math.log(1.0 + math.sqrt(2.0))
HBM_PEAK = 8.0e12  # bytes/s, MI355X nominal


def step_floor_bytes(L, tile=64):
    """1 B spin read + 4 B label write (local) + 4 B label read + 1 B spin read + 1 B spin write (resolve) per site, plus the
    merge: per seam bond 2 spin bytes + 2 labels read (periodic: L / tile seams each way)."""
    sites = L * L
    seam_bonds = 2 * (L // tile) * L
    return sites * 11 + seam_bonds * (2 + 8)


def time_steps(L, T, n_steps, warm=3):
    ctx = _hip.Context.default()
    lat = _hip.Lattice(L, L, True, ctx=ctx)
    if T < TC:
        lat.fill(1)
    else:
        lat.randomize(1)
    lat.cluster_sweep(1.0, T, warm, 7, 0)
    ctx.synchronize()
    ctx.timer_begin()
    lat.cluster_sweep(1.0, T, n_steps, 7, warm)
    ms = ctx.timer_end() / n_steps
    launches = lat.cluster_launch_count() / (warm + n_steps)
    lat.close()
    return ms, launches


def tau_int(x, c=6.0):
    x = np.asarray(x, float) - np.mean(x)
    n = len(x)
    f = np.fft.rfft(x, 2 * n)
    acf = np.fft.irfft(f * np.conj(f))[:n]
    acf /= acf[0]
    tau = 0.5
    for w in range(1, n):
        tau += acf[w]
        if w >= c * tau:
            break
    return tau


def autocorrelation(L, n_sw, n_hb, every):
    m = IsingModel2D(L, temperature=TC, seed=17)
    m.cluster_update(1000)
    ctx = _hip.Context.default()
    sw = np.empty(n_sw)
    ctx.synchronize()
    t0 = time.perf_counter()
    for i in range(n_sw):
        m.cluster_update(1)
        sw[i] = abs(m.magnetization())
    sw_wall = (time.perf_counter() - t0) / n_sw
    ctx.timer_begin()
    m.cluster_update(200)
    sw_ms = ctx.timer_end() / 200
    hb = np.empty(n_hb)
    for i in range(n_hb):
        m.gibbs_update(every)
        hb[i] = abs(m.magnetization())
    ctx.timer_begin()
    m.gibbs_update(2000)
    hb_ms = ctx.timer_end() / 2000
    t_sw, t_hb = tau_int(sw), every * tau_int(hb)
    return {"L": L, "tau_sw_steps": t_sw, "tau_hb_sweeps": t_hb, "ratio": t_hb / t_sw, "sw_ms_per_step": sw_ms,
            "hb_ms_per_sweep": hb_ms, "sw_ms_per_independent": 2 * t_sw * sw_ms, "hb_ms_per_independent": 2 * t_hb * hb_ms,
            "sw_wall_ms_per_measured_step": 1e3 * sw_wall, "n_sw": n_sw, "n_hb": n_hb, "hb_every": every}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--steps-only", action="store_true")
    ap.add_argument("--sizes", default="1024,4096,8192,16384")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    lines, res = [], {"steps": [], "autocorrelation": []}
    info = _hip.Context.default().device_info()
    lines.append(f"device: {info['name']}, {info['compute_units']} CUs")
    lines.append("ms per SW step (periodic L x L, J = 1; device events over n steps after 3 warm-up steps)")
    lines.append(f"{'L':>6} {'T':>7} {'ms/step':>9} {'floor MB':>9} {'floor GB/s':>10} {'of 8 TB/s':>9} {'launches/step':>13}")
    for L in [int(x) for x in a.sizes.split(",")]:
        for T in (2.0, TC, 3.0):
            n = 20 if L <= 4096 else 8
            ms, launches = time_steps(L, T, n)
            fb = step_floor_bytes(L)
            gbs = fb / (ms * 1e-3) / 1e9
            res["steps"].append({"L": L, "T": T, "ms_per_step": ms, "floor_bytes": fb, "floor_GBps": gbs,
                                 "floor_fraction_of_peak": gbs * 1e9 / HBM_PEAK, "launches": launches})
            lines.append(f"{L:>6} {T:>7.4f} {ms:>9.3f} {fb / 1e6:>9.1f} {gbs:>10.1f} {gbs * 1e9 / HBM_PEAK:>9.3f} {launches:>13g}")
            print(lines[-1], flush=True)
    if not a.steps_only:
        lines.append("")
        lines.append("tau_int(|m|) at T_c, periodic L x L (Sokal window c = 6); time per independent sample = 2 tau x time per step")
        lines.append(f"{'L':>5} {'tau SW':>8} {'tau HB':>9} {'ratio':>7} {'SW ms/step':>10} {'HB ms/sweep':>11} "
                     f"{'SW ms/indep':>11} {'HB ms/indep':>11}")
        for L, n_sw, n_hb, every in ((64, 20000, 20000, 4), (128, 20000, 20000, 8), (256, 20000, 30000, 16)):
            r = autocorrelation(L, n_sw, n_hb, every)
            res["autocorrelation"].append(r)
            lines.append(f"{L:>5} {r['tau_sw_steps']:>8.2f} {r['tau_hb_sweeps']:>9.1f} {r['ratio']:>7.1f} {r['sw_ms_per_step']:>10.4f} "
                         f"{r['hb_ms_per_sweep']:>11.4f} {r['sw_ms_per_independent']:>11.4f} {r['hb_ms_per_independent']:>11.3f}")
            print(lines[-1], flush=True)
    name = "cluster_time_steps" if a.steps_only else "cluster_time"
    with open(os.path.join(a.out, name + ".txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(a.out, name + ".json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

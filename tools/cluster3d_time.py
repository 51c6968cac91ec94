"""K8 Swendsen-Wang in 3-D: us per step by cube size and temperature (device events, medians of 5 after a warm-up of every
shape), sites/s, the step's byte floor and the fraction of the HBM peak it reaches, k8_sweep's us per sweep in the same run,
and at 64^3 and T_c the integrated autocorrelation time of |m| under both and the time per independent sample.

    python tools/cluster3d_time.py [--out DIR] [--steps-only] [--sizes 32,64,128,256]

--steps-only skips the autocorrelation part (the command a rocprofv3 --kernel-trace --stats run profiles).  Writes
DIR/cluster3d_time.txt and DIR/cluster3d_time.json (default DIR: profiles/)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))
from tsu import _hip  # noqa: E402
from tsu.models.ising import IsingModel3D  # noqa: E402

TC3 = 4.5115
HBM_PEAK = 8.0e12  # bytes/s, MI355X nominal
SMALL_SITES = 16384


def default_tile(L, cus):
    """The library's choice: 16 x 32 x 32 once that many tiles fill the chip, 8 x 16 x 32 below (None: one workgroup)."""
    if L ** 3 <= SMALL_SITES:
        return None
    big = -(-L // 16) * -(-L // 32) * -(-L // 32)
    return (16, 32, 32) if big >= cus else (8, 16, 32)


def step_floor_bytes(L, tile):
    """Per site: 1 B spin + 3 x 4 B couplings read and a 4 B label written (local), a 4 B label chased and 1 B spin read and
    written (resolve): 23 B.  Per seam bond of the periodic cube (merge): 2 spin bytes, a 4 B coupling and 2 labels: 14 B.
    One workgroup (no tile): the spins in and out once per call, the couplings every step from L2: nothing from HBM per step."""
    if tile is None:
        return 0
    seams = sum(-(-L // t) for t in tile) * L * L
    return L ** 3 * 23 + seams * 14


def median_us(ctx, call, n_inner, reps=5):
    out = []
    for _ in range(reps):
        ctx.synchronize()
        ctx.timer_begin()
        call(n_inner)
        out.append(1e3 * ctx.timer_end() / n_inner)  # timer_end synchronises
    return float(np.median(out))


def time_cube(L, T):
    ctx = _hip.Context.default()
    m = IsingModel3D(L, temperature=T, seed=1, initial="up" if T < TC3 else "random")
    n = 40 if L <= 64 else (10 if L <= 128 else 4)
    m.cluster_update(3 * n)  # warm-up of this shape (and towards equilibrium)
    m.gibbs_update(3)
    sw = median_us(ctx, m.cluster_update, n)
    hb = median_us(ctx, m.gibbs_update, n)
    launches = m._lat.cluster_launch_count() / m.cluster_count
    return sw, hb, launches


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
    ctx = _hip.Context.default()
    m = IsingModel3D(L, temperature=TC3, seed=17)
    m.cluster_update(1000)
    sw = np.empty(n_sw)
    for i in range(n_sw):
        m.cluster_update(1)
        sw[i] = abs(m.magnetization())
    sw_us = median_us(ctx, m.cluster_update, 100)
    hb = np.empty(n_hb)
    for i in range(n_hb):
        m.gibbs_update(every)
        hb[i] = abs(m.magnetization())
    hb_us = median_us(ctx, m.gibbs_update, 500)
    t_sw, t_hb = tau_int(sw), every * tau_int(hb)
    return {"L": L, "tau_sw_steps": t_sw, "tau_hb_sweeps": t_hb, "ratio": t_hb / t_sw, "sw_us_per_step": sw_us,
            "hb_us_per_sweep": hb_us, "sw_us_per_independent": 2 * t_sw * sw_us, "hb_us_per_independent": 2 * t_hb * hb_us,
            "n_sw": n_sw, "n_hb": n_hb, "hb_every": every}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--steps-only", action="store_true")
    ap.add_argument("--sizes", default="32,64,128,256")
    ap.add_argument("--tau", default="64", help="cube sizes of the autocorrelation part")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    lines, res = [], {"steps": [], "autocorrelation": []}
    info = _hip.Context.default().device_info()
    cus = info["compute_units"]
    lines.append(f"device: {info['name']}, {cus} CUs")
    lines.append("us per SW step and per k8_sweep sweep (periodic L^3, J = 1; medians of 5 timings by device events after a warm-up)")
    lines.append(f"{'L':>4} {'T':>7} {'tile':>9} {'SW us/step':>10} {'Msites/s':>9} {'floor MB':>9} {'floor GB/s':>10} {'of 8 TB/s':>9} "
                 f"{'launches/step':>13} {'HB us/sweep':>11}")
    for L in [int(x) for x in a.sizes.split(",") if x]:
        tile = default_tile(L, cus)
        for T in (4.0, TC3, 5.0):
            sw, hb, launches = time_cube(L, T)
            fb = step_floor_bytes(L, tile)
            gbs = fb / (sw * 1e-6) / 1e9
            res["steps"].append({"L": L, "T": T, "tile": tile, "sw_us_per_step": sw, "sites_per_s": L ** 3 / (sw * 1e-6),
                                 "floor_bytes": fb, "floor_GBps": gbs, "floor_fraction_of_peak": gbs * 1e9 / HBM_PEAK,
                                 "launches_per_step": launches, "hb_us_per_sweep": hb})
            tname = "one WG" if tile is None else "x".join(str(t) for t in tile)
            lines.append(f"{L:>4} {T:>7.4f} {tname:>9} {sw:>10.1f} {L ** 3 / sw:>9.1f} {fb / 1e6:>9.2f} {gbs:>10.1f} "
                         f"{gbs * 1e9 / HBM_PEAK:>9.4f} {launches:>13.3g} {hb:>11.1f}")
            print(lines[-1], flush=True)
    if not a.steps_only:
        lines.append("")
        lines.append("tau_int(|m|) at T_c, periodic L^3 (Sokal window c = 6); time per independent sample = 2 tau x time per update")
        lines.append(f"{'L':>4} {'tau SW':>8} {'tau HB':>9} {'ratio':>7} {'SW us/step':>10} {'HB us/sweep':>11} {'SW us/indep':>11} "
                     f"{'HB us/indep':>11} {'HB / SW':>8}")
        for L in [int(x) for x in a.tau.split(",") if x]:
            r = autocorrelation(L, 20000, 20000, 8 if L <= 32 else 32)
            res["autocorrelation"].append(r)
            lines.append(f"{L:>4} {r['tau_sw_steps']:>8.2f} {r['tau_hb_sweeps']:>9.1f} {r['ratio']:>7.1f} {r['sw_us_per_step']:>10.1f} "
                         f"{r['hb_us_per_sweep']:>11.1f} {r['sw_us_per_independent']:>11.1f} {r['hb_us_per_independent']:>11.1f} "
                         f"{r['hb_us_per_independent'] / r['sw_us_per_independent']:>8.1f}")
            print(lines[-1], flush=True)
    name = "cluster3d_time_steps" if a.steps_only else "cluster3d_time"
    with open(os.path.join(a.out, name + ".txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(a.out, name + ".json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

"""K8 ghost-spin Swendsen-Wang steps: us per step by cube size and temperature for the zero-field entry point and for the ghost entry
point at h = 0, at uniform h = 0.05 and at random h = +-0.5 (device events, medians of 5 rounds that alternate between the four
after a warm-up of each), the cost of the ghost pass (ghost entry point at h = 0 over the zero-field one), and at 32^3, T_c and
h = 0.01 the integrated autocorrelation time of the signed m under ghost steps and under heat-bath sweeps.

    python tools/cluster_field_time.py [--out DIR] [--steps-only] [--sizes 64,128,256]

Writes DIR/cluster_field_time.txt and DIR/cluster_field_time.json (default DIR: profiles/)."""
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
VARIANTS = ("zero-field entry", "ghost, h = 0", "ghost, h = 0.05", "ghost, h = +-0.5")


def once_us(ctx, call, n_inner):
    ctx.synchronize()
    ctx.timer_begin()
    call(n_inner)
    return 1e3 * ctx.timer_end() / n_inner  # timer_end synchronises


def time_cube(L, T, rounds=5):
    """us per step of the four variants: medians over `rounds` rounds, each round timing the four in turn."""
    ctx = _hip.Context.default()
    initial = "up" if T < TC3 else "random"
    plain = IsingModel3D(L, temperature=T, seed=1, initial=initial)
    uniform = IsingModel3D(L, temperature=T, seed=1, initial=initial, external_field=0.05)
    h = np.random.default_rng(L).choice(np.array([-0.5, 0.5], np.float32), size=(L, L, L))
    random = IsingModel3D(L, temperature=T, seed=1, initial=initial, field=h)
    calls = (plain.cluster_update, plain.ghost_cluster_update, uniform.ghost_cluster_update, random.ghost_cluster_update)
    n = 40 if L <= 64 else (10 if L <= 128 else 4)
    for call in calls:
        call(3 * n)  # warm-up of this shape and kernel (and towards equilibrium)
    t = np.array([[once_us(ctx, call, n) for call in calls] for _ in range(rounds)])
    return np.median(t, axis=0)


def tau_int(x, c=6.0):
    """integrated autocorrelation time with Sokal's automatic window"""
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


def autocorrelation(L, h, n_sw, n_hb, every):
    m = IsingModel3D(L, temperature=TC3, seed=17, external_field=h)
    m.ghost_cluster_update(1000)
    sw = np.empty(n_sw)
    for i in range(n_sw):
        m.ghost_cluster_update(1)
        sw[i] = m.magnetization()
    hb = np.empty(n_hb)
    for i in range(n_hb):
        m.gibbs_update(every)
        hb[i] = m.magnetization()
    t_sw, t_hb = tau_int(sw), every * tau_int(hb)
    return {"L": L, "h": h, "tau_ghost_steps": t_sw, "tau_hb_sweeps": t_hb, "ratio": t_hb / t_sw, "m_ghost": float(sw.mean()),
            "m_hb": float(hb.mean()), "n_sw": n_sw, "n_hb": n_hb, "hb_every": every}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--steps-only", action="store_true")
    ap.add_argument("--sizes", default="64,128,256")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    lines, res = [], {"steps": [], "autocorrelation": []}
    info = _hip.Context.default().device_info()
    lines.append(f"device: {info['name']}, {info['compute_units']} CUs")
    lines.append("us per cluster step (periodic L^3, J = 1; medians of 5 rounds alternating between the four columns, device events, "
                 "after a warm-up of each)")
    lines.append(f"{'L':>4} {'T':>7} " + " ".join(f"{v:>17}" for v in VARIANTS) + f" {'ghost pass (2/1)':>17}")
    for L in [int(x) for x in a.sizes.split(",") if x]:
        for T in (4.0, TC3, 5.0):
            us = time_cube(L, T)
            res["steps"].append({"L": L, "T": T, "us_per_step": dict(zip(VARIANTS, (float(u) for u in us))),
                                 "ghost_pass_ratio": float(us[1] / us[0])})
            lines.append(f"{L:>4} {T:>7.4f} " + " ".join(f"{u:>17.1f}" for u in us) + f" {us[1] / us[0]:>17.3f}")
            print(lines[-1], flush=True)
    if not a.steps_only:
        r = autocorrelation(32, 0.01, 20000, 20000, 8)
        res["autocorrelation"].append(r)
        lines.append("")
        lines.append("tau_int(m) of the signed magnetisation at T_c and uniform h = 0.01, periodic 32^3 (Sokal window c = 6)")
        lines.append(f"{'L':>4} {'tau ghost steps':>15} {'tau HB sweeps':>13} {'ratio':>7} {'<m> ghost':>10} {'<m> HB':>10}")
        lines.append(f"{r['L']:>4} {r['tau_ghost_steps']:>15.2f} {r['tau_hb_sweeps']:>13.1f} {r['ratio']:>7.1f} {r['m_ghost']:>10.4f} "
                     f"{r['m_hb']:>10.4f}")
        print(lines[-1], flush=True)
    with open(os.path.join(a.out, "cluster_field_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(a.out, "cluster_field_time.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

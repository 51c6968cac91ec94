"""Cluster-size records: what a measured Swendsen-Wang step costs and what the improved estimator buys.

For 64^2, 4096^2 (K6), 64^3 and 256^3 (K8), each below T_c, at T_c and above: us per plain step and per measured step of one
model (device events, medians of 5 rounds that alternate between the two after a warm-up of each), their ratio r, and at 64^3 the
variance ratio v = Var(sum_m2) / Var(plain M^2 of the same steps) at T_c and at T = 5.0.  A measured step pays per independent
sample of <M^2> where r v < 1.

    python tools/cluster_measure_time.py [--out DIR] [--cases 2:64,2:4096,3:64,3:256] [--no-variance] [--plain-only]

--plain-only times the unmeasured steps alone (the run to compare against another build of the library); --cases with one case
and --no-variance is the command for a rocprofv3 --kernel-trace --stats run of the extra kernels.  Writes
DIR/cluster_measure_time.txt (default DIR: profiles/; an existing parent comparison below the marker line is kept)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))
from tsu import _hip  # noqa: E402
from tsu.models.ising import IsingModel2D, IsingModel3D  # noqa: E402

TC = {2: 2.269185, 3: 4.5115}
TEMPS = {2: (2.0, TC[2], 2.6), 3: (4.0, TC[3], 5.0)}
MARKER = "plain steps, parent commit against this tree"


def make(dim, L, T):
    cls = IsingModel2D if dim == 2 else IsingModel3D
    return cls(L, temperature=T, seed=1, initial="up" if T < TC[dim] else "random")


def once_us(ctx, call, n_inner):
    ctx.synchronize()
    ctx.timer_begin()
    call(n_inner)
    return 1e3 * ctx.timer_end() / n_inner  # timer_end synchronises


def time_case(dim, L, T, plain_only, rounds=5):
    ctx = _hip.Context.default()
    m = make(dim, L, T)
    n = 40 if L ** dim <= 64 ** 3 else 4
    calls = [lambda k: m.cluster_update(k)] + ([] if plain_only else [lambda k: m.cluster_update(k, measure=True)])
    for call in calls:
        call(3 * n)  # warm-up of this shape and kernel (and towards equilibrium)
    t = np.array([[once_us(ctx, call, n) for call in calls] for _ in range(rounds)])
    launches = m._lat.cluster_launch_count()
    calls[-1](1)
    return np.median(t, axis=0), m._lat.cluster_launch_count() - launches


def variance_ratio(L, T, n_steps=2000, drop=300):
    m = make(3, L, T)
    imp, plain = np.empty(n_steps), np.empty(n_steps)
    for i in range(n_steps):
        m.cluster_update(1, measure=True)
        imp[i] = float(int(m.cluster_record()["sum_m2"][0]))
        plain[i] = float(m._lat.sum_spins()) ** 2
    return float(np.var(imp[drop:], ddof=1) / np.var(plain[drop:], ddof=1)), float(np.mean(imp[drop:])), float(np.mean(plain[drop:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--cases", default="2:64,2:4096,3:64,3:256")
    ap.add_argument("--no-variance", action="store_true")
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    info = _hip.Context.default().device_info()
    lines = [f"device: {info['name']}, {info['compute_units']} CUs",
             "us per Swendsen-Wang step of one periodic lattice, J = 1 (medians of 5 rounds alternating between the columns, device events, "
             "after a warm-up of each); launches: per measured step (per call on the one-workgroup route)"]
    lines.append(f"{'lattice':>8} {'T':>7} {'plain':>10}" + ("" if a.plain_only else f" {'measured':>10} {'r':>7} {'launches':>9}"))
    r_of = {}
    for case in [c for c in a.cases.split(",") if c]:
        dim, L = (int(x) for x in case.split(":"))
        for T in TEMPS[dim]:
            us, launches = time_case(dim, L, T, a.plain_only)
            name = f"{L}^{dim}"
            if a.plain_only:
                lines.append(f"{name:>8} {T:>7.4f} {us[0]:>10.1f}")
            else:
                r_of[(dim, L, T)] = us[1] / us[0]
                lines.append(f"{name:>8} {T:>7.4f} {us[0]:>10.1f} {us[1]:>10.1f} {us[1] / us[0]:>7.3f} {launches:>9}")
            print(lines[-1], flush=True)
    if not (a.no_variance or a.plain_only):
        lines += ["", "64^3: v = Var(sum_m2) / Var(plain M^2 of the same steps), 2000 single measured steps, the first 300 dropped; "
                  "r from the table; a measured step pays per independent sample of <M^2> where r v < 1",
                  f"{'T':>7} {'v':>7} {'r':>7} {'r v':>7} {'<sum_m2>':>14} {'<M^2>':>14}"]
        for T in (TC[3], 5.0):
            v, mi, mp = variance_ratio(64, T)
            r = r_of.get((3, 64, T), float("nan"))
            lines.append(f"{T:>7.4f} {v:>7.3f} {r:>7.3f} {r * v:>7.3f} {mi:>14.1f} {mp:>14.1f}")
            print(lines[-1], flush=True)
    path = os.path.join(a.out, "cluster_measure_time.txt")
    kept = []
    if os.path.exists(path) and not a.plain_only:
        with open(path) as f:
            old = f.read().split("\n")
        at = [i for i, l in enumerate(old) if l.startswith(MARKER)]
        kept = [""] + old[at[0]:] if at else []
    if a.plain_only:
        path = os.path.join(a.out, "cluster_measure_time_plain.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines + kept).rstrip("\n") + "\n")


if __name__ == "__main__":
    main()

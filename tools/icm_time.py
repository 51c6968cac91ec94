"""K7 replica cluster moves (Houdayer) inside the tempering ladder: what a pass costs and what it buys.

  (a) microseconds per pass and bytes/s against the byte floor (14 B per site and slot: local 2 B read + 4 B label written,
      resolve 4 B label + 2 B read + up to 2 B written) at 64^2 x 32, 1024^2 x 16 and 4096^2 x 16 slots, +-J couplings, ladder
      0.3 ... 2.0, every slot taking part, after 20 sweeps from a random start; the one-workgroup route where the lattice fits,
      the tiled route (TSU_ICM_TILE=64 forces it at 64^2) everywhere, with the fraction of sites a pass flipped per slot.
  (b) 32^2 +-J, 16 temperatures 0.2 ... 1.6, two ladders, one sweep per round: the integrated autocorrelation time (Sokal's
      window, c = 6) of q and of ladder 0's energy at the four coldest slots, and the round trips per 10^4 rounds, with
      cluster_moves=1 and with cluster_moves=0 (the same seeds).

    python tools/icm_time.py --part a|b [--out DIR] [--rounds N]

Each part keeps its lines in DIR/icm_time.json and re-renders DIR/icm_time.txt from both (default DIR: profiles/)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))
from tsu import _hip  # noqa: E402
from tsu.models.ising import LatticeTempering  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X nominal
FLOOR = 14.0       # bytes per site and slot of a tiled pass
SEED_J, SEED = 1, 3


def pm_j(L, seed=SEED_J):
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], size=(L, L)).astype(np.float32), rng.choice([-1.0, 1.0], size=(L, L)).astype(np.float32))


def tau_int(x, c=6.0):
    """integrated autocorrelation time with Sokal's automatic window (the rule of tests/test_cluster_gpu.py)"""
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


def part_a():
    ctx = _hip.Context.default()
    lines = [f"(a) one pass over every slot; +-J (seed {SEED_J}), T = 0.3 ... 2.0, ladder seed {SEED}, after 20 sweeps from a random start; "
             f"floor = {FLOOR:.0f} B per site and slot, HBM peak {HBM_PEAK / 1e12:.1f} TB/s"]
    for L, R, routes in ((64, 32, ("small", "tiled")), (1024, 16, ("tiled",)), (4096, 16, ("tiled",))):
        pt = LatticeTempering(L, np.linspace(0.3, 2.0, R), couplings=pm_j(L), seed=SEED, ladders=2, cluster_moves=1)
        try:
            pt.run(2, 10, swap=True, record=False)  # two passes on the way
            for route in routes:
                if route == "tiled" and L * L <= 16384:
                    os.environ["TSU_ICM_TILE"] = "64"
                n = 200 if L <= 1024 else 20
                pt.cluster_move()
                ctx.synchronize()
                before = pt.cluster_stats
                ctx.timer_begin()
                for _ in range(n):
                    pt.cluster_move()
                us = ctx.timer_end() * 1e3 / n
                os.environ.pop("TSU_ICM_TILE", None)
                after = pt.cluster_stats
                frac = (after["flipped"] - before["flipped"]) / (n * float(L * L))
                ncl = (after["clusters"] - before["clusters"]) / n
                bw = FLOOR * L * L * R / (us * 1e-6)
                lines.append(f"{L}^2 x {R} slots, {route:5s}: {us:10.1f} us/pass  {L * L * R / (us * 1e-6):.3e} sites/s  floor {bw / 1e12:.3f} TB/s = "
                             f"{bw / HBM_PEAK:.3f} of HBM peak  clusters/slot {ncl.min():.0f} ... {ncl.max():.0f}  flipped fraction "
                             f"{frac.min():.3f} ... {frac.max():.3f} (coldest {frac[0]:.3f}, hottest {frac[-1]:.3f})")
                print(lines[-1], flush=True)
        finally:
            pt._pt.close()
    return lines


def part_b(rounds):
    L, R, n_eq = 32, 16, max(2000, rounds // 10)
    Ts = np.linspace(0.2, 1.6, R)
    lines = [f"(b) {L}^2 +-J (seed {SEED_J}), T = 0.2 ... 1.6 in {R} steps, two ladders, ladder seed {SEED}, one sweep per round, "
             f"{n_eq} rounds discarded, {rounds} measured; tau in rounds (Sokal window, c = 6)"]
    res = {}
    for cm in (1, 0):
        pt = LatticeTempering(L, Ts, couplings=pm_j(L), seed=SEED, ladders=2, cluster_moves=cm)
        try:
            pt.run(n_eq, 1, record=False)
            trips0 = pt.round_trips
            q, e = [], []
            chunk = 50000
            for lo in range(0, rounds, chunk):
                h = pt.run(min(chunk, rounds - lo), 1)
                q.append(h["q"][:, :4] / float(L * L))
                e.append(h["E"][:, :4] / float(L * L))
            q, e = np.concatenate(q), np.concatenate(e)
            st = pt.cluster_stats
            res[cm] = dict(tau_q=[tau_int(q[:, i]) for i in range(4)], tau_e=[tau_int(e[:, i]) for i in range(4)],
                           q2=[float(np.mean(q[:, i] ** 2)) for i in range(4)], e=[float(np.mean(e[:, i])) for i in range(4)],
                           trips=(pt.round_trips - trips0) * 1e4 / rounds, acc=pt.acceptance,
                           flipped=st["flipped"] / np.maximum(st["passes"], 1) / float(L * L))
        finally:
            pt._pt.close()
    for i in range(4):
        on, off = res[1], res[0]
        lines.append(f"slot {i} (T = {Ts[i]:.3f}): tau_int(q) {off['tau_q'][i]:9.1f} without, {on['tau_q'][i]:9.1f} with cluster moves, ratio "
                     f"{off['tau_q'][i] / on['tau_q'][i]:5.2f};  tau_int(E) {off['tau_e'][i]:8.1f} without, {on['tau_e'][i]:8.1f} with, ratio "
                     f"{off['tau_e'][i] / on['tau_e'][i]:5.2f};  <q^2> {off['q2'][i]:.4f} / {on['q2'][i]:.4f}  <E>/N {off['e'][i]:.4f} / {on['e'][i]:.4f}")
    lines.append(f"round trips per 10^4 rounds (all 32 walkers): {res[0]['trips']:.1f} without, {res[1]['trips']:.1f} with cluster moves;  "
                 f"lowest swap acceptance {np.nanmin(res[0]['acc']):.3f} / {np.nanmin(res[1]['acc']):.3f}")
    lines.append("flipped fraction per pass and slot, coldest first: " + " ".join(f"{x:.3f}" for x in res[1]["flipped"]))
    for ln in lines:
        print(ln, flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("a", "b"), required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--rounds", type=int, default=200000, help="measured rounds of part (b)")
    a = ap.parse_args()
    lines = part_a() if a.part == "a" else part_b(a.rounds)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "icm_time.json")
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc[a.part] = lines
    doc["device"] = _hip.Context.default().device_info()
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
    with open(os.path.join(a.out, "icm_time.txt"), "w") as f:
        for part in ("a", "b"):
            f.write("\n".join(doc.get(part, [])) + "\n")


if __name__ == "__main__":
    main()

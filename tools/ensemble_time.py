"""Tempering ensembles: the time of a round of 10 sweeps for S disorder samples in one handle (LatticeTemperingEnsemble /
LatticeTemperingEnsemble3D, periodic lattices, Gaussian J, swaps on) against the same samples as standalone ladders run back to
back in the same process, which is the only route without the ensembles and so the yardstick.  Device events around calls that
end in a synchronise, every handle warmed up, medians of 5.  Per case (lattice, temperatures, ladders) and S:

  round           us per round of all S samples (run(swap=True, record=False)), and that divided by S
  sweeps          us per round with swap=False, record=False: the half-sweep launches alone, and the walker-updates/s they make
  energy + swap   round - sweeps: the energy partial and final passes and the swap pass, as a share of the recorded round
  recording       recorded round - round: q, L (two ladders), profiles and modes, as a share of the recorded round
  W               the walker group of the sweep launches (pt_group_of on S nl R walkers, clamped to nl R)
  ladders         min(S, 64) standalone ladders of the same samples and seeds, each run(...) enqueued one after the other, one
                  synchronise at the end: us per round and ladder (it does not depend on how many there are), and ladder / ensemble
                  per sample.  A ratio below 1.1 is reported as "not faster".

Every case runs in a child process of its own under a time limit; the first one that fails or runs out of time ends the tool.

    python tools/ensemble_time.py [--out DIR] [--cases 3d:8x16x2,3d:16x32x1,3d:16x32x2,2d:64x32x2] [--samples 1,8,64,256]

Writes DIR/ensemble_time.txt and DIR/ensemble_time.json (default DIR: profiles/).

    rocprofv3 --kernel-trace --stats --output-format csv -- python tools/ensemble_time.py --trace

runs nothing but one warm-up round and one recorded round (10 sweeps, swaps, q, L, profiles, modes) of 16^3 x 32 T x 2 ladders x 64
samples in this process: the workload of profiles/ensemble_round_16x16x16x32x2_S64_kernel_stats.csv."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))

THETA = 10
REPS = 5
MARGIN = 1.1
MAX_LADDERS = 64
CASE_SECONDS = 240


def median_ms(ctx, call, per):
    out = []
    for _ in range(REPS):
        ctx.timer_begin()
        call()
        out.append(ctx.timer_end() / per)
    return float(np.median(out))


def group_of(cus, lanes, walkers, per_sample):
    """pt_group_of (csrc/pt_host.h) without TSU_PT_GROUP, clamped to a sample's walkers."""
    groups = -(-(cus if cus > 0 else 256) * 1024 // lanes)
    w = 1 if groups >= walkers else -(-walkers // groups)
    return min(w, per_sample)


def one_case(dim, L, R, nl, S):
    """Runs on the GPU (a child process): the row of one case as a dict."""
    from tsu import _hip
    from tsu.models import ising
    ctx = _hip.Context.default()
    os.environ.pop("TSU_PT_GROUP", None)
    shape, N = (L,) * dim, L ** dim
    js = ising.edwards_anderson_samples(shape, S, kind="gaussian", seed=1, dims=dim)
    Ts = np.linspace(2.0, 0.5, R)
    seeds = ising.ensemble_seeds(3, S, nl, R)
    flags = dict(ladders=nl, correlation=True, link_overlap=nl == 2)
    ens_cls, lad_cls = ((ising.LatticeTemperingEnsemble, ising.LatticeTempering) if dim == 2 else
                        (ising.LatticeTemperingEnsemble3D, ising.LatticeTempering3D))
    n = max(1, min(8, int(2e9 / (N * S * nl * R * THETA))))
    ens = ens_cls(shape, Ts, couplings=js, seeds=seeds, **flags)
    try:
        ms = {}
        for key, swap, record in (("sweeps", False, False), ("round", True, False), ("recorded", True, True)):
            ens._pt.run(n, THETA, swap, record)
            ctx.synchronize()
            ms[key] = median_ms(ctx, lambda: (ens._pt.run(n, THETA, swap, record), ctx.synchronize()), n)
    finally:
        ens.close()
    n_lad = min(S, MAX_LADDERS)
    lads = [lad_cls(shape, Ts, couplings=tuple(a[s] for a in js), seed=seeds[s], **flags) for s in range(n_lad)]
    try:
        def all_ladders():
            for pt in lads:
                pt._pt.run(n, THETA, True, False)
            ctx.synchronize()
        all_ladders()
        ms_ladder = median_ms(ctx, all_ladders, n * n_lad)
    finally:
        for pt in lads:
            pt._pt.close()
    info = ctx.device_info()
    lanes = (N // L) * (-(-L // 16))
    ratio = ms_ladder / (ms["round"] / S)
    return dict(dim=dim, L=L, temperatures=R, ladders=nl, samples=S, walkers=S * nl * R, rounds_per_call=n,
                W=group_of(info["compute_units"], lanes, S * nl * R, nl * R), us_round=ms["round"] * 1e3,
                us_round_per_sample=ms["round"] * 1e3 / S, us_sweeps=ms["sweeps"] * 1e3, us_recorded_round=ms["recorded"] * 1e3,
                energy_swap_share=(ms["round"] - ms["sweeps"]) / ms["recorded"], recording_share=(ms["recorded"] - ms["round"]) / ms["recorded"],
                walker_updates_per_s=N * S * nl * R * THETA / (ms["sweeps"] * 1e-3), standalone_ladders=n_lad,
                us_ladder_round=ms_ladder * 1e3, ladder_over_ensemble=ratio, faster=bool(ratio > MARGIN), device=info)


def traced_round():
    from tsu import _hip
    from tsu.models import ising
    js = ising.edwards_anderson_samples((16,) * 3, 64, kind="gaussian", seed=1)
    ens = ising.LatticeTemperingEnsemble3D((16,) * 3, np.linspace(2.0, 0.5, 32), couplings=js, seed=3, ladders=2, correlation=True,
                                           link_overlap=True)
    try:
        ens.run(1, THETA)
        ens.run(1, THETA)
        _hip.Context.default().synchronize()
    finally:
        ens.close()


def line_of(r):
    verdict = f"{r['ladder_over_ensemble']:.2f}x" if r["faster"] else f"{r['ladder_over_ensemble']:.2f}x: not faster (margin {MARGIN})"
    return (f"{r['L']}^{r['dim']} x {r['temperatures']} T x {r['ladders']} ladder(s), S = {r['samples']:3d} ({r['walkers']} walkers, W = {r['W']}): "
            f"round {r['us_round']:9.1f} us = {r['us_round_per_sample']:7.1f} per sample; sweeps {r['us_sweeps']:9.1f} "
            f"({r['walker_updates_per_s']:.3e} walker-updates/s); recorded round {r['us_recorded_round']:9.1f}: energy + swap "
            f"{r['energy_swap_share']:.3f}, recording {r['recording_share']:.3f} | standalone ladder {r['us_ladder_round']:7.1f} us per round: "
            f"{verdict}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--cases", default="3d:8x16x2,3d:16x32x1,3d:16x32x2,2d:64x32x2")
    ap.add_argument("--samples", default="1,8,64,256")
    ap.add_argument("--child", default=None, help="internal: dim,L,R,ladders,S of the one case this process measures")
    ap.add_argument("--trace", action="store_true", help="one warm-up and one recorded round at 16^3 x 32 x 2, S = 64, nothing else")
    a = ap.parse_args()
    if a.trace:
        traced_round()
        return 0
    if a.child:
        print("ROW " + json.dumps(one_case(*(int(x) for x in a.child.split(",")))), flush=True)
        return 0
    rows, lines = [], []
    for case in a.cases.split(","):
        d, rest = case.split(":")
        L, R, nl = (int(x) for x in rest.split("x"))
        for S in (int(x) for x in a.samples.split(",")):
            if S * nl * R > 65535:
                continue
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{d[0]},{L},{R},{nl},{S}"], capture_output=True,
                                   text=True, timeout=CASE_SECONDS)
            except subprocess.TimeoutExpired:
                print(f"{case} S = {S}: no result within {CASE_SECONDS} s; stopping", flush=True)
                return 1
            got = [ln[4:] for ln in p.stdout.splitlines() if ln.startswith("ROW ")]
            if p.returncode != 0 or not got:
                print(f"{case} S = {S}: exit status {p.returncode}; stopping\n{p.stderr[-2000:]}", flush=True)
                return 1
            rows.append(json.loads(got[0]))
            lines.append(line_of(rows[-1]))
            print(lines[-1], flush=True)
    os.makedirs(a.out, exist_ok=True)
    device = rows[0].pop("device") if rows else None
    for r in rows[1:]:
        r.pop("device", None)
    with open(os.path.join(a.out, "ensemble_time.json"), "w") as f:
        json.dump(dict(theta=THETA, reps=REPS, margin=MARGIN, device=device, rows=rows), f, indent=1)
    with open(os.path.join(a.out, "ensemble_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""K14, population annealing of Potts lattices with stored couplings: the time of a step of 10 heat-bath sweeps of a population
(16^2, 32^2, 8^3 and 16^3; q = 3 and 8; with and without a Gaussian site field; R = 256 and 16384 walkers) on
  (a) the route the shipped packing rule gives it (k14_pop_pack where it packs),
  (b) the same handle with TSU_POTTS_POP_PACK=0 (k14_pop_small, one workgroup per walker),
  (c) K13's ladder of 256 walkers on the same disorder, swap=False, record=False (K13 is unchanged: the parent's rate),
and the share of a step spent in plan + copy and in the measuring pass; one 4096^2 x 8 line on k14_pop_sweep.  The candidates are
timed in turn, round after round, in one process, so that whatever else the machine does hits them alike; the table gives the median
of the rounds and their range.  Also the registers, LDS and scratch of every K14 kernel from the compiler's resource remarks.

    python tools/potts_pop_time.py [--out DIR] [--no-resources | --resources-only] [--commit LABEL] [--quick]

Host clock around work that ends in a device synchronise, after one warm-up round of each.  Writes DIR/potts_pop_time.txt (default
DIR: profiles/); --resources-only replaces the resource table of an existing file and needs no GPU."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tsu import _hip  # noqa: E402
from potts_disorder_time import FLAGS, HIPCC, kernel_resources  # noqa: E402

ROUNDS = 5
SWEEPS = 10
LADDER = 256
MARK = "kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)"


def _disorder(shape, q, field, rng):
    J = [rng.standard_normal(size=shape, dtype=np.float32) for _ in shape]
    h = rng.standard_normal(size=(q,) + tuple(shape), dtype=np.float32) if field else None
    return J, h


def _timed(ctx, fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def one_shape(shape, R, q, field, say, ladder=True):
    rng = np.random.default_rng(1)
    sites = int(np.prod(shape))
    J, h = _disorder(shape, q, field, rng)
    n_steps = 5 * (ROUNDS + 1)
    betas = np.linspace(0.8, 1.25, n_steps + 1)  # T about 1 throughout; every step resamples a little
    pa = _hip.PottsPopulation(shape, q, True, R)
    pa.set_disorder(J[0], J[1], J[2] if len(J) == 3 else None, h)
    pa.set_schedule(betas)
    pa.init(7, _hip.POTTS_POP_DRAW, 0)
    ctx = pa.ctx
    pt = None
    if ladder:
        pt = _hip.PottsTemperingLattice(shape, q, True, LADDER, 1)
        pt.set_disorder(J[0], J[1], J[2] if len(J) == 3 else None, h)
        pt.set_temperatures(np.full(LADDER, 1.0))
        pt.init(7, -1)
        for g in range(LADDER):
            pt.set_spins(0, g, pa.get_spins(g % R))
    del J, h

    def step(sweeps, resample, pack):
        if not pack:
            os.environ["TSU_POTTS_POP_PACK"] = "0"
        try:
            pa.run(1, sweeps, resample, False)
        finally:
            os.environ.pop("TSU_POTTS_POP_PACK", None)

    shipped = pa.plan()
    cands = [("a", lambda: step(SWEEPS, True, True)), ("b", lambda: step(SWEEPS, True, False)), ("a0", lambda: step(SWEEPS, False, True)),
             ("m", lambda: step(0, False, True))]
    if ladder:
        cands.append(("c", lambda: pt.run(1, SWEEPS, False, False)))
    times = {name: [] for name, _ in cands}
    for k in range(ROUNDS + 1):  # round 0 warms up every kernel and path
        for name, fn in cands:
            dt = _timed(ctx, fn)
            if k:
                times[name].append(dt)
    pa.close()
    if pt:
        pt.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    rate = lambda name, n: n * sites * SWEEPS / (med[name] * 1e-3)  # noqa: E731
    name = "x".join(map(str, shape)) + f" x {R}"
    c_ms = f"{med['c']:9.3f}" if ladder else f"{'-':>9}"
    c_rate = f"{rate('c', LADDER):10.3e}" if ladder else f"{'-':>10}"
    say(f"{name:>16} {q:>2} {'yes' if field else 'no':>5} {shipped['route'][4:]:>9} {shipped['G']:>3} {shipped['lds_bytes']:>6} {med['a']:>9.3f} {med['b']:>9.3f} "
        f"{c_ms} {rate('a', R):>10.3e} {rate('b', R):>10.3e} {c_rate} {med['b'] / med['a']:>6.2f} {100 * (med['a'] - med['a0']) / med['a']:>6.1f} "
        f"{100 * med['m'] / med['a']:>6.1f}  " + " ".join(f"{k} {min(v):.3f}..{max(v):.3f}" for k, v in times.items()))
    # (a) slower than (b) beyond the range of the rounds: every round of (a) above every round of (b)
    return shipped["route"] == "k14_pop_pack" and min(times["a"]) > max(times["b"])


def resources(say):
    csrc = os.path.join(ROOT, "tsu-emulator_amd", "csrc")
    say(MARK + ": the kernels of csrc/potts_pop.hip")
    say(f"{'kernel':>40} {'VGPRs':>6} {'AGPRs':>6} {'SGPRs':>6} {'scratch B/lane':>14} {'LDS B':>7} {'waves/SIMD':>10}")
    for k, v in kernel_resources(csrc, "potts_pop.hip", r"^k14_|^pop_plan|^pop_copy|^pop_identity|^k13_pt_final").items():
        say(f"{k:>40} " + " ".join(f"{x:>{w}}" for x, w in zip(v, (6, 6, 6, 14, 7, 10))))
    say("k14_pop_pack declares its LDS at launch (potts_pop_plan.h: at most 65536 B a workgroup); k13_pt_small under its launch bound of 1024:")
    for k, v in kernel_resources(csrc, "potts_pt.hip", r"^k13_pt_small").items():
        say(f"{k:>40} " + " ".join(f"{x:>{w}}" for x, w in zip(v, (6, 6, 6, 14, 7, 10))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--commit", default="unknown", help="a label of the source state, written into the file")
    ap.add_argument("--quick", action="store_true", help="R = 256 only and a small HBM lattice (a check of the tool itself)")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "potts_pop_time.txt")
    lines = []

    def say(s=""):
        lines.append(s)
        print(s, flush=True)

    if a.resources_only:
        old = open(path).read().split(MARK)[0].rstrip("\n").splitlines() if os.path.exists(path) else []
        resources(say)
        with open(path, "w") as f:
            f.write("\n".join(old + [""] + lines if old else lines) + "\n")
        return
    info = _hip.Context.default().device_info()
    ver = subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout.splitlines()
    say(f"device: {info['name']}, {info['compute_units']} CUs")
    say(f"compiler: {ver[0] if ver else HIPCC}; {' '.join(FLAGS[:3])} (csrc/build.sh)")
    say(f"source: {a.commit}")
    say(f"a step = plan + copy, {SWEEPS} heat-bath sweeps of every walker at T about 1, one measuring pass; no record; periodic lattices, Gaussian")
    say(f"couplings (and field), device draw; host clock to a device synchronise, one warm-up round, then the median of {ROUNDS} rounds, timed in turn")
    say("(a) the shipped route; (b) the same handle with TSU_POTTS_POP_PACK=0; (c) K13's ladder of 256 walkers, swap=False, record=False (sweeps only);")
    say("u/s: walkers sites 10 / time; b/a: time of (b) over time of (a); res %: share of (a) in plan + copy ((a) minus a step without them);")
    say("meas %: a step of no sweeps and no resampling (the measuring pass alone) over (a)")
    say(f"{'lattice x R':>16} {'q':>2} {'field':>5} {'route':>9} {'G':>3} {'LDS B':>6} {'(a) ms':>9} {'(b) ms':>9} {'(c) ms':>9} {'(a) u/s':>10} {'(b) u/s':>10} {'(c) u/s':>10} "
        f"{'b/a':>6} {'res %':>6} {'meas %':>6}  ranges of the rounds (ms)")
    slower = []
    for shape in ((16, 16), (32, 32), (8, 8, 8), (16, 16, 16)):
        for q in (3, 8):
            for field in (False, True):
                for R in (256,) if a.quick else (256, 16384):
                    if one_shape(shape, R, q, field, say):
                        slower.append(("x".join(map(str, shape)), q, field, R))
    one_shape((256, 256) if a.quick else (4096, 4096), 8, 3, False, say, ladder=False)
    say()
    if slower:
        say("the shipped rule packs shapes where every round of (a) is slower than every round of (b): " + ", ".join(map(str, slower)))
    else:
        say("the shipped rule sends no shape to k14_pop_pack where (a) is slower than (b) beyond the range of the rounds")
    say("not measured: the pack kernel with the disorder left in global memory (only the LDS-staged form exists in the source)")
    if not a.no_resources:
        say()
        resources(say)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""K13, parallel tempering of Potts lattices with stored couplings: the time of a round of 10 heat-bath sweeps with a swap pass on the
ladder handle (64^2 x 32 temperatures and 16^3 x 32 on k13_pt_small, 4096^2 x 8 and 256^3 x 4 on k13_pt_sweep; Gaussian couplings,
q = 3 and 8, with and without a Gaussian site field) beside, in the same run and on the same disorder and temperatures,
  (a) the walker-by-walker loop a user writes without the handle: R K12 handles, 10 sweeps each, every energy fetched to the host,
      the swap pass on the host;
  (b) the R K12 sweep calls of (a) alone, enqueued back to back: K12's own updates per second per walker.
The three are timed in turn, round after round, so that whatever else the machine does hits them alike; the table gives the median
of the rounds and their range.  Also the registers, LDS and scratch of every K13 kernel from the compiler's resource remarks.

    python tools/potts_pt_time.py [--out DIR] [--no-resources] [--commit LABEL] [--quick]

Host clock around work that ends in a device synchronise, after one warm-up round of each; one process.  Writes
DIR/potts_pt_time.txt (default DIR: profiles/)."""
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


def _disorder(shape, q, field, rng):
    J = [rng.standard_normal(size=shape, dtype=np.float32) for _ in shape]
    h = rng.standard_normal(size=(q,) + tuple(shape), dtype=np.float32) if field else None
    return J, h


def _host_swap_pass(was, T, E, rng):
    """The pass of the contract on the host (NumPy's uniforms: this loop is timed, not compared)."""
    for i in range(len(was) - 1):
        a, b = was[i], was[i + 1]
        delta = (1.0 / T[i] - 1.0 / T[i + 1]) * (E[a] - E[b])
        if delta >= 0 or rng.random() < np.exp(delta):
            was[i], was[i + 1] = b, a


def one_shape(shape, R, q, field, say):
    rng = np.random.default_rng(1)
    sites = int(np.prod(shape))
    T = np.linspace(0.8, 1.6, R)
    J, h = _disorder(shape, q, field, rng)
    pt = _hip.PottsTemperingLattice(shape, q, True, R, 1)
    pt.set_disorder(J[0], J[1], J[2] if len(J) == 3 else None, h)
    pt.set_temperatures(T)
    pt.init(7, -1)
    lats = []
    for g in range(R):
        s = np.random.default_rng(7 + g).integers(0, q, size=shape).astype(np.int8)
        pt.set_spins(0, g, s)
        lat = _hip.PottsDisorderLattice(shape, q, True)
        lat.set_disorder(J[0], J[1], J[2] if len(J) == 3 else None, h)
        lat.set_spins(s)
        lats.append(lat)
    del J, h
    ctx = pt.ctx
    was = list(range(R))
    swap_rng = np.random.default_rng(3)
    state = {"sweep0": 0}

    def ladder():
        pt.run(1, SWEEPS, True, False)
        ctx.synchronize()

    def sweeps_only():
        for i, w in enumerate(was):
            lats[w].sweep(float(T[i]), SWEEPS, 7 + w, state["sweep0"])
        ctx.synchronize()

    def loop():
        for i, w in enumerate(was):
            lats[w].sweep(float(T[i]), SWEEPS, 7 + w, state["sweep0"])
        E = [lat.measure()[2] for lat in lats]
        _host_swap_pass(was, T, E, swap_rng)

    times = {"ladder": [], "loop": [], "k12": []}
    for k in range(ROUNDS + 1):  # round 0 warms up every kernel and path
        for name, fn in (("ladder", ladder), ("loop", loop), ("k12", sweeps_only)):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if name != "ladder":
                state["sweep0"] += SWEEPS
            if k:
                times[name].append(dt * 1e3)
    route, launches = pt.route(), pt.launch_count() // (ROUNDS + 1)
    pt.close()
    for lat in lats:
        lat.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    rate = {k: R * sites * SWEEPS / (med[k] * 1e-3) for k in med}
    name = "x".join(map(str, shape)) + f" x {R}"
    say(f"{name:>16} {q:>2} {'yes' if field else 'no':>5} {route:>13} {launches:>4} {med['ladder']:>9.3f} {med['loop']:>9.3f} {med['k12']:>9.3f} "
        f"{rate['ladder']:>10.3e} {rate['k12']:>10.3e} {med['loop'] / med['ladder']:>7.2f} {rate['ladder'] / rate['k12']:>7.3f}  "
        + " ".join(f"{k} {min(v):.3f}..{max(v):.3f}" for k, v in times.items()))
    return med["loop"] / med["ladder"], rate["ladder"] / rate["k12"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--commit", default="unknown", help="a label of the source state, written into the file")
    ap.add_argument("--quick", action="store_true", help="small lattices only (a check of the tool itself)")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    info = _hip.Context.default().device_info()
    ver = subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout.splitlines()
    lines = [f"device: {info['name']}, {info['compute_units']} CUs", f"compiler: {ver[0] if ver else HIPCC}; {' '.join(FLAGS[:3])} (csrc/build.sh)",
             f"source: {a.commit}"]

    def say(s=""):
        lines.append(s)
        print(s, flush=True)

    say(f"a round = {SWEEPS} heat-bath sweeps of every walker + one swap pass; periodic lattices, Gaussian couplings (and field), T = 0.8 .. 1.6,")
    say(f"random start; host clock to a device synchronise, one warm-up round, then the median of {ROUNDS} rounds, the three timed in turn")
    say("ladder: tsu_potts_pt_run(1, 10, swap, no record); loop: R K12 handles, sweep(10) each, measure() each on the host, swap on the host;")
    say("k12: the loop's R sweep calls alone, back to back; updates/s: R sites 10 / time; launches: the ladder's per round")
    say(f"{'lattice x R':>16} {'q':>2} {'field':>5} {'route':>13} {'ln':>4} {'ladder ms':>9} {'loop ms':>9} {'k12 ms':>9} {'ladder u/s':>10} {'k12 u/s':>10} "
        f"{'loop/lad':>7} {'lad/k12':>7}  ranges of the rounds (ms)")
    small = [((64, 64), 32), ((16, 16, 16), 32)]
    big = [((256, 256), 8), ((32, 32, 32), 4)] if a.quick else [((4096, 4096), 8), ((256, 256, 256), 4)]
    worst_small, worst_big = float("inf"), float("inf")
    for shape, R in small + big:
        for q in (3, 8):
            for field in (False, True):
                speedup, ratio = one_shape(shape, R, q, field, say)
                if (shape, R) in small:
                    worst_small = min(worst_small, speedup)
                else:
                    worst_big = min(worst_big, ratio)
    say()
    say(f"small route: the ladder round is at least {worst_small:.2f} x faster than the walker-by-walker loop (must be > 1)")
    say(f"HBM route: the ladder's walker-updates/s, swap pass included, are at least {worst_big:.3f} x K12's own (must be >= 0.9)")
    if not a.no_resources:
        csrc = os.path.join(ROOT, "tsu-emulator_amd", "csrc")
        say()
        say("kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): the kernels of csrc/potts_pt.hip")
        say(f"{'kernel':>34} {'VGPRs':>6} {'AGPRs':>6} {'SGPRs':>6} {'scratch B/lane':>14} {'LDS B':>7} {'waves/SIMD':>10}")
        for k, v in kernel_resources(csrc, "potts_pt.hip", r"^k13_|^k7_pt_swap").items():
            say(f"{k:>34} " + " ".join(f"{x:>{w}}" for x, w in zip(v, (6, 6, 6, 14, 7, 10))))
    with open(os.path.join(a.out, "potts_pt_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

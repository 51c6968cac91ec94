"""K11 multicanonical Potts walkers: walker-updates per second of k11_muca on its three routes and with several workgroup sizes,
beside k10_sweep on the same total number of sites in the same run; the registers, LDS and scratch of the kernels from the compiler's
resource remarks; and, for 2-D q = 8 at L = 16 and 32, the weight iterations until the histogram is flat over the full range and the
tunnel events per walker with the converged weights.

    python tools/potts_muca_time.py [--out DIR] [--no-resources] [--no-convergence] [--commit LABEL]

Device events after warm-up; one process.  Writes DIR/potts_muca_time.txt and DIR/potts_muca_time.json (default DIR: profiles/)."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))
from tsu import _hip  # noqa: E402
from tsu.models.potts_muca import PottsMulticanonical, muca_flatness  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ROUTE_ENV, BLOCK_ENV = "TSU_POTTS_MUCA_ROUTE", "TSU_POTTS_MUCA_BLOCK"


def _timed(ctx, fn):
    ctx.synchronize()
    ctx.timer_begin()
    fn()
    return ctx.timer_end()  # ms


def muca_rate(shape, q, walkers, T, n_sweeps, route=None, block=None):
    """(walker-updates per second, route) with canonical weights ln W = n / T from a random start."""
    for name, v in ((ROUTE_ENV, route), (BLOCK_ENV, block)):
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(v)
    try:
        h = _hip.PottsMucaWalkers(*shape, q, walkers, True)
        h.set_weights(np.arange(h.bonds + 1) / T)
        h.set_spins(np.random.default_rng(1).integers(0, q, size=(walkers,) + tuple(shape)).astype(np.int8))
        h.run(2, 7, 0)
        ms = _timed(h.ctx, lambda: h.run(n_sweeps, 7, 2))
        ok, name = h.measure(), h.route()
        h.close()
    finally:
        os.environ.pop(ROUTE_ENV, None)
        os.environ.pop(BLOCK_ENV, None)
    assert ok, "the incremental n_eq differs from a recount"
    return walkers * shape[0] * shape[1] * shape[2] * n_sweeps / (ms * 1e-3), name


def k10_rate(L, q, n, warm=3):
    ctx = _hip.Context.default()
    lat = _hip.PottsLattice(L, L, q, True, ctx=ctx)
    lat.set_spins(np.random.default_rng(1).integers(0, q, size=(L, L)).astype(np.int8))
    T = 1.0 / np.log(1.0 + np.sqrt(q))
    lat.sweep(T, warm, 7, 0)
    ms = _timed(ctx, lambda: lat.sweep(T, n, 7, warm))
    lat.close()
    return L * L * n / (ms * 1e-3)


def kernel_resources():
    """VGPRs, LDS and scratch of the k11 kernels as hipcc's -Rpass-analysis=kernel-resource-usage states them."""
    src = os.path.join(ROOT, "tsu-emulator_amd", "csrc", "potts_muca.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", os.devnull], capture_output=True, text=True)
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"k11_(muca|measure)", m.group(1))
            name = k.group(0) if k else None
            if name == "k11_muca":
                name += {"ILb1ELb1E": "<lds>", "ILb0ELb1E": "<global>", "ILb0ELb0E": "<atomics>"}.get(re.search(r"ILb\dELb\dE", m.group(1)).group(0), "")
            if name:
                out.setdefault(name, {})
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def convergence(L, q, walkers, sweeps_per_iteration, max_iterations, n_production):
    """Weight iterations from ln W = 0 and all walkers ordered until the record covers 0 .. B with flatness >= 0.5; then a production
    run with the weights fixed, tunnel events counted between n_eq <= 0.4 B and n_eq >= 0.95 B (below the disordered and above the
    ordered peak of 2-D q = 8 at its transition, n / B = 0.46 and 0.91)."""
    m = PottsMulticanonical(L, q, walkers, seed=5)
    B = m.bonds
    t0 = time.time()
    its, done = [], None
    for k in range(max_iterations):
        info = m.iterate(sweeps_per_iteration)
        its.append({"range": list(info["range"]), "flatness": info["flatness"], "holes": info["holes"]})
        if info["range"] == (0, B) and info["flatness"] >= 0.5:
            done = k + 1
            break
    m.set_tunnel_bounds(int(0.4 * B), int(0.95 * B))
    m.clear_record().run(n_production)
    lo, hi, flat, holes = muca_flatness(m.histogram())
    events = m.tunnels()
    out = {"L": L, "q": q, "walkers": walkers, "route": m.route(), "sweeps_per_iteration": sweeps_per_iteration, "iterations_to_flat": done,
           "iterations_run": len(its), "iterations": its, "production_sweeps": n_production, "production_range": [lo, hi],
           "production_flatness": flat, "production_holes": holes, "tunnel_bounds": [int(0.4 * B), int(0.95 * B)],
           "tunnels_per_walker_per_1000_sweeps": float(events.mean() * 1000.0 / n_production), "walkers_that_tunnelled": int((events > 0).sum()),
           "consistent": m.consistent(), "seconds": time.time() - t0}
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--no-convergence", action="store_true")
    ap.add_argument("--commit", default="unknown", help="a label of the source state, written into the files")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    info = _hip.Context.default().device_info()
    lines = [f"device: {info['name']}, {info['compute_units']} CUs", "build: hipcc --offload-arch=gfx950 -O3 (csrc/build.sh)", f"source: {a.commit}"]
    res = {"device": info["name"], "source": a.commit, "rates": [], "k10": [], "resources": {}, "convergence": []}

    def say(s=""):
        lines.append(s)
        print(s, flush=True)

    say("k11_muca, periodic lattices, canonical weights ln W = n / T at T = T_c(q) (2-D) or 1.8163 (3-D q = 3), random start;")
    say("walker-updates per second from device events after 2 warm-up sweeps; 'auto' is the route and workgroup size the library picks;")
    say("a forced workgroup size that does not fit the LDS is ignored (16 x 16 on the lds route: 1024)")
    say(f"{'lattice':>10} {'q':>2} {'walkers':>8} {'sweeps':>6} {'setting':>22} {'route':>17} {'updates/s':>11}")
    for shape, q, walkers, n in (((1, 16, 16), 8, 65536, 40), ((1, 32, 32), 8, 16384, 20), ((1, 64, 64), 8, 4096, 10), ((16, 16, 16), 3, 4096, 10)):
        T = 1.8163 if shape[0] > 1 else 1.0 / np.log(1.0 + np.sqrt(q))
        settings = [("auto", None, None), ("route >= global", 1, None), ("route = atomics", 2, None)]
        settings += [(f"auto, block {b}", None, b) for b in (64, 128, 256, 512, 1024)]
        for label, route, block in settings:
            rate, name = muca_rate(shape, q, walkers, T, n, route, block)
            res["rates"].append({"shape": shape, "q": q, "walkers": walkers, "sweeps": n, "setting": label, "route": name, "updates_per_s": rate})
            say(f"{'x'.join(map(str, shape[1:] if shape[0] == 1 else shape)):>10} {q:>2} {walkers:>8} {n:>6} {label:>22} {name:>17} {rate:>11.3e}")
    say()
    say("the yardstick of the same run: k10_sweep (checkerboard heat bath), periodic 4096 x 4096 = the same 2^24 sites, T = T_c(q), three rounds")
    for q in (8, 3):
        rates = [k10_rate(4096, q, 10) for _ in range(3)]
        res["k10"].append({"L": 4096, "q": q, "updates_per_s": rates})
        say(f"{'k10_sweep':>10} {q:>2} " + " ".join(f"{v:>11.3e}" for v in rates))
    if not a.no_resources:
        res["resources"] = kernel_resources()
        say()
        say("kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950); the LDS is dynamic: 62 (B + 1) bytes of histogram and")
        say("table on the lds and global routes, plus sites x workgroup bytes of lattices on the lds route")
        say(f"{'kernel':>18} {'VGPRs':>6} {'SGPRs':>6} {'LDS B (static)':>14} {'scratch B/lane':>14} {'waves/SIMD':>10}")
        for k, v in sorted(res["resources"].items()):
            say(f"{k:>18} {v.get('vgprs', -1):>6} {v.get('sgprs', -1):>6} {v.get('lds', -1):>14} {v.get('scratch', -1):>14} {v.get('occupancy', -1):>10}")
    if not a.no_convergence:
        say()
        say("weight recursion, 2-D q = 8, periodic, from ln W = 0 and ordered walkers: iterations until the record covers 0 .. B with")
        say("flatness (min / mean of H over the visited bins) >= 0.5; then tunnel events between n_eq <= 0.4 B and n_eq >= 0.95 B")
        for L, walkers, spi, max_it, n_prod in ((16, 16384, 200, 60, 2000), (32, 4096, 500, 80, 2000)):
            c = convergence(L, 8, walkers, spi, max_it, n_prod)
            res["convergence"].append(c)
            say(f"L = {L}, {walkers} walkers, {spi} sweeps per iteration, route {c['route']}: flat after "
                f"{c['iterations_to_flat'] if c['iterations_to_flat'] else 'more than ' + str(c['iterations_run'])} iterations "
                f"(last: range {c['iterations'][-1]['range']}, flatness {c['iterations'][-1]['flatness']:.3f}, holes {c['iterations'][-1]['holes']})")
            say(f"    production, {n_prod} sweeps: range {c['production_range']}, flatness {c['production_flatness']:.3f}, "
                f"{c['tunnels_per_walker_per_1000_sweeps']:.3f} tunnel events per walker per 1000 sweeps, {c['walkers_that_tunnelled']} walkers "
                f"tunnelled, n_eq consistent: {c['consistent']}, {c['seconds']:.1f} s in all")
    with open(os.path.join(a.out, "potts_muca_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(a.out, "potts_muca_time.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

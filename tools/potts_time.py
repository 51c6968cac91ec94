"""K10 Potts lattices: time per heat-bath sweep of k10_small and k10_sweep beside k7_sweep on constant arrays, time per
Swendsen-Wang step beside K6 (three alternating rounds, so that the run-to-run spread is on the page), and the registers, LDS and
scratch of the new kernels from the compiler's resource remarks.

    python tools/potts_time.py [--out DIR] [--no-resources]

Device events after warm-up; one process, so the yardsticks are measured in the same run.  Writes DIR/potts_time.txt and
DIR/potts_time.json (default DIR: profiles/)."""
import argparse
import json
import math
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))
from tsu import _hip  # noqa: E402

TC_ISING = 2.0 / math.log(1.0 + math.sqrt(2.0))


def tc(q):
    return 1.0 / math.log(1.0 + math.sqrt(q))


def _timed(ctx, fn, n):
    ctx.synchronize()
    ctx.timer_begin()
    fn(n)
    return 1e3 * ctx.timer_end() / n  # us per update


def potts_sweep_us(L, q, n, warm=3):
    ctx = _hip.Context.default()
    lat = _hip.PottsLattice(L, L, q, True, ctx=ctx)
    lat.set_spins(np.random.default_rng(1).integers(0, q, size=(L, L)).astype(np.int8))
    lat.sweep(tc(q), warm, 7, 0)
    us = _timed(ctx, lambda k: lat.sweep(tc(q), k, 7, warm), n)
    route = lat.route()
    lat.close()
    return us, route


def k7_sweep_us(L, n, warm=3):
    ctx = _hip.Context.default()
    lat = _hip.Lattice(L, L, True, ctx=ctx)
    lat.randomize(1)
    one = np.ones((L, L), np.float32)
    lat.set_disorder(one, one, 0 * one)
    lat.disorder_sweep(TC_ISING, warm, 7, 0)
    us = _timed(ctx, lambda k: lat.disorder_sweep(TC_ISING, k, 7, warm), n)
    lat.close()
    return us


def potts_step_us(L, q, n, warm=3):
    ctx = _hip.Context.default()
    lat = _hip.PottsLattice(L, L, q, True, ctx=ctx)
    lat.set_spins(np.random.default_rng(1).integers(0, q, size=(L, L)).astype(np.int8))
    lat.cluster_sweep(tc(q), warm, 7, 0)
    us = _timed(ctx, lambda k: lat.cluster_sweep(tc(q), k, 7, warm), n)
    lat.close()
    return us


def k6_step_us(L, n, warm=3):
    ctx = _hip.Context.default()
    lat = _hip.Lattice(L, L, True, ctx=ctx)
    lat.randomize(1)
    lat.cluster_sweep(1.0, TC_ISING, warm, 7, 0)
    us = _timed(ctx, lambda k: lat.cluster_sweep(1.0, TC_ISING, k, 7, warm), n)
    lat.close()
    return us


def kernel_resources():
    """VGPRs, LDS and scratch of the k10 kernels as hipcc's -Rpass-analysis=kernel-resource-usage states them."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "tsu-emulator_amd", "csrc", "potts2d.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", os.devnull], capture_output=True, text=True)
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = re.search(r"k10_[a-z_]+", m.group(1))  # potts2d.hip instantiates potts_kern_dev.h's templates at DIM = 2 only
            name = name.group(0) if name else None
            if name == "k10_sweep":  # its two instantiations: rows of whole octets (16-byte loads) or any width (byte loads)
                name += "<rows16>" if "Lb1E" in m.group(1) else "<bytes>"
            if name == "k10_sw_small" and "SwRecOut" in m.group(1):
                name = None  # the measured instantiation sw_host.h names; never launched
            if name:
                out.setdefault(name, {})
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--no-resources", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    lines, res = [], {"small": [], "sweep": [], "cluster": [], "resources": {}}
    info = _hip.Context.default().device_info()
    lines.append(f"device: {info['name']}, {info['compute_units']} CUs")
    lines.append("heat-bath sweeps, periodic L x L, J = 1, zero field, T = T_c(q), random start (device events after 3 warm-up sweeps)")
    lines.append(f"{'kernel':>10} {'L':>5} {'q':>2} {'us/sweep':>10} {'updates/s':>10}")
    for L in (64, 128):
        for q in (3, 8):
            us, route = potts_sweep_us(L, q, 2000)
            res["small"].append({"L": L, "q": q, "us_per_sweep": us, "updates_per_s": L * L / us * 1e6, "route": route})
            lines.append(f"{route:>10} {L:>5} {q:>2} {us:>10.3f} {L * L / us * 1e6:>10.3e}")
            print(lines[-1], flush=True)
    for L in (1024, 4096):
        n = 40 if L == 1024 else 10
        for q in (3, 8):
            us, route = potts_sweep_us(L, q, n)
            res["sweep"].append({"L": L, "q": q, "us_per_sweep": us, "updates_per_s": L * L / us * 1e6, "route": route})
            lines.append(f"{route:>10} {L:>5} {q:>2} {us:>10.1f} {L * L / us * 1e6:>10.3e}")
            print(lines[-1], flush=True)
        us = k7_sweep_us(L, n)
        res["sweep"].append({"L": L, "q": 2, "us_per_sweep": us, "updates_per_s": L * L / us * 1e6, "route": "k7_sweep"})
        lines.append(f"{'k7_sweep':>10} {L:>5} {'-':>2} {us:>10.1f} {L * L / us * 1e6:>10.3e}   (constant J = 1, h = 0, T = 2.269)")
        print(lines[-1], flush=True)
    lines.append("")
    lines.append("Swendsen-Wang steps at T_c, periodic L x L: Potts q = 3 beside K6 (Ising), three alternating rounds, us per step")
    lines.append(f"{'L':>5} {'k10 r1':>9} {'k6 r1':>9} {'k10 r2':>9} {'k6 r2':>9} {'k10 r3':>9} {'k6 r3':>9} {'k10/k6 (medians)':>17}")
    for L in (64, 1024, 4096):
        n = 400 if L == 64 else (20 if L == 1024 else 8)
        rounds = [(potts_step_us(L, 3, n), k6_step_us(L, n)) for _ in range(3)]
        ratio = float(np.median([r[0] for r in rounds]) / np.median([r[1] for r in rounds]))
        res["cluster"].append({"L": L, "k10_us": [r[0] for r in rounds], "k6_us": [r[1] for r in rounds], "ratio": ratio})
        lines.append(f"{L:>5} " + " ".join(f"{v:>9.1f}" for r in rounds for v in r) + f" {ratio:>17.3f}")
        print(lines[-1], flush=True)
    if not a.no_resources:
        res["resources"] = kernel_resources()
        lines.append("")
        lines.append("kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)")
        lines.append(f"{'kernel':>18} {'VGPRs':>6} {'SGPRs':>6} {'LDS B (static)':>14} {'scratch B/lane':>14}")
        for k, v in sorted(res["resources"].items()):
            lines.append(f"{k:>18} {v.get('vgprs', -1):>6} {v.get('sgprs', -1):>6} {v.get('lds', -1):>14} {v.get('scratch', -1):>14}")
            print(lines[-1], flush=True)
        lines.append("(dynamic LDS on top: k10_sw_small 5 B a site, k10_sw_local 5 B a tile site = 20480 B at the 64 x 64 tile)")
    with open(os.path.join(a.out, "potts_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(a.out, "potts_time.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

"""K10 Potts lattices in 3-D: time per heat-bath sweep of k10_3d_small and k10_3d_sweep beside k8_sweep on constant arrays at the
same shape, time per Swendsen-Wang step beside K8's cluster step at the same shape and T / T_c, k10_sweep at 4096 x 4096 as the 2-D
yardstick of the same run, and the registers, LDS and scratch of the new kernels from the compiler's resource remarks.

    python tools/potts3d_time.py [--out DIR] [--no-resources] [--commit LABEL]

Device events after warm-up; one process, three alternating rounds per pair, so the yardsticks are measured in the same run and the
run-to-run spread is on the page.  Writes DIR/potts3d_time.txt and DIR/potts3d_time.json (default DIR: profiles/)."""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))
from tsu import _hip  # noqa: E402

T_Q3 = 1.8163     # q = 3 on the cubic lattice, in units of J; q = 8 is timed at the same temperature
TC_ISING3D = 4.5115
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _timed(ctx, fn, n):
    ctx.synchronize()
    ctx.timer_begin()
    fn(n)
    return 1e3 * ctx.timer_end() / n  # us per update


def _potts(shape, q):
    lat = _hip.PottsLattice3D(shape[0], shape[1], shape[2], q, True, ctx=_hip.Context.default())
    lat.set_spins(np.random.default_rng(1).integers(0, q, size=shape).astype(np.int8))
    return lat


def _ising(shape):
    lat = _hip.Lattice3D(shape[0], shape[1], shape[2], True, ctx=_hip.Context.default())
    lat.randomize(1)
    one = np.ones(shape, np.float32)
    lat.set_disorder(one, one, one)
    return lat


def potts_sweep_us(shape, q, n, warm=3):
    lat = _potts(shape, q)
    lat.sweep(T_Q3, warm, 7, 0)
    us = _timed(lat.ctx, lambda k: lat.sweep(T_Q3, k, 7, warm), n)
    route = lat.route()
    lat.close()
    return us, route


def k8_sweep_us(shape, n, warm=3):
    lat = _ising(shape)
    lat.sweep(TC_ISING3D, warm, 7, 0)
    us = _timed(lat.ctx, lambda k: lat.sweep(TC_ISING3D, k, 7, warm), n)
    lat.close()
    return us


def potts_step_us(shape, q, n, warm=3):
    lat = _potts(shape, q)
    lat.cluster_sweep(T_Q3, warm, 7, 0)
    us = _timed(lat.ctx, lambda k: lat.cluster_sweep(T_Q3, k, 7, warm), n)
    route = lat.route(_hip.POTTS_SWENDSEN_WANG)
    lat.close()
    return us, route


def k8_step_us(shape, n, warm=3):
    lat = _ising(shape)
    lat.cluster_sweep(TC_ISING3D, warm, 7, 0)
    us = _timed(lat.ctx, lambda k: lat.cluster_sweep(TC_ISING3D, k, 7, warm), n)
    lat.close()
    return us


def k10_2d_sweep_us(L, q, n, warm=3):
    ctx = _hip.Context.default()
    lat = _hip.PottsLattice(L, L, q, True, ctx=ctx)
    lat.set_spins(np.random.default_rng(1).integers(0, q, size=(L, L)).astype(np.int8))
    T = 1.0 / np.log(1.0 + np.sqrt(q))
    lat.sweep(T, warm, 7, 0)
    us = _timed(ctx, lambda k: lat.sweep(T, k, 7, warm), n)
    lat.close()
    return us


def kernel_resources():
    """VGPRs, LDS and scratch of the k10_3d kernels as hipcc's -Rpass-analysis=kernel-resource-usage states them."""
    src = os.path.join(ROOT, "tsu-emulator_amd", "csrc", "potts3d.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", os.devnull], capture_output=True, text=True)
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            # potts3d.hip instantiates potts_kern_dev.h's templates at DIM = 3 only; the labels keep the 3-D route names' prefix
            name = re.search(r"k10_[a-z_]+", m.group(1))
            name = name.group(0).replace("k10_", "k10_3d_") if name else None
            if name == "k10_3d_sweep":  # its two instantiations: rows of whole octets (16-byte loads) or any width (byte loads)
                name += "<rows16>" if "Lb1E" in m.group(1) else "<bytes>"
            if name == "k10_3d_sw_small" and "SwRecOut" in m.group(1):
                name = None  # the measured instantiation sw_host.h names; never launched
            if name:
                out.setdefault(name, {})
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def _hipcc_version():
    try:
        r = subprocess.run([HIPCC, "--version"], capture_output=True, text=True)
        return next((line.strip() for line in r.stdout.splitlines() if "HIP version" in line), "unknown")
    except OSError:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--commit", default="unknown", help="a label of the source state, written into the files")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    info = _hip.Context.default().device_info()
    build = f"hipcc {_hipcc_version()}, --offload-arch=gfx950 -O3 (csrc/build.sh)"
    lines = [f"device: {info['name']}, {info['compute_units']} CUs", f"build: {build}", f"source: {a.commit}"]
    res = {"device": info["name"], "build": build, "source": a.commit, "sweep": [], "cluster": [], "k10_2d": [], "resources": {}}
    lines.append("heat-bath sweeps, periodic D x R x C, J = 1, zero field, T = 1.8163, random start; k8_sweep: constant J = 1, h = 0, T = 4.5115")
    lines.append("device events after 3 warm-up sweeps, three alternating rounds (q = 3, q = 8, k8), us per sweep; updates/s from the medians")
    lines.append(f"{'shape':>12} {'route':>13} " + " ".join(f"{f'q3 r{i}':>8} {f'q8 r{i}':>8} {f'k8 r{i}':>8}" for i in (1, 2, 3))
                 + f" {'q3 upd/s':>10} {'q8 upd/s':>10} {'k8 upd/s':>10}")
    for shape, n in (((16, 16, 16), 2000), ((24, 24, 28), 1000), ((64, 64, 64), 200), ((128, 128, 128), 40), ((256, 256, 256), 10)):
        sites = shape[0] * shape[1] * shape[2]
        rounds, route = [], None
        for _ in range(3):
            u3, route = potts_sweep_us(shape, 3, n)
            u8, _ = potts_sweep_us(shape, 8, n)
            rounds.append((u3, u8, k8_sweep_us(shape, n)))
        med = [float(np.median([r[k] for r in rounds])) for k in range(3)]
        res["sweep"].append({"shape": shape, "route": route, "q3_us": [r[0] for r in rounds], "q8_us": [r[1] for r in rounds],
                             "k8_us": [r[2] for r in rounds], "updates_per_s": [sites / m * 1e6 for m in med]})
        lines.append(f"{'x'.join(map(str, shape)):>12} {route:>13} " + " ".join(f"{v:>8.1f}" for r in rounds for v in r)
                     + " " + " ".join(f"{sites / m * 1e6:>10.3e}" for m in med))
        print(lines[-1], flush=True)
    lines.append("")
    lines.append("Swendsen-Wang steps at T / T_c = 1, periodic: Potts q = 3 (T = 1.8163) beside K8 (constant J = 1, T = 4.5115), three alternating rounds, us per step")
    lines.append(f"{'shape':>12} {'route':>16} {'k10 r1':>9} {'k8 r1':>9} {'k10 r2':>9} {'k8 r2':>9} {'k10 r3':>9} {'k8 r3':>9} {'k10/k8 (medians)':>17}")
    for shape, n in (((16, 16, 16), 400), ((24, 24, 28), 200), ((64, 64, 64), 40), ((128, 128, 128), 10), ((256, 256, 256), 4)):
        rounds, route = [], None
        for _ in range(3):
            us, route = potts_step_us(shape, 3, n)
            rounds.append((us, k8_step_us(shape, n)))
        ratio = float(np.median([r[0] for r in rounds]) / np.median([r[1] for r in rounds]))
        res["cluster"].append({"shape": shape, "route": route, "k10_us": [r[0] for r in rounds], "k8_us": [r[1] for r in rounds], "ratio": ratio})
        lines.append(f"{'x'.join(map(str, shape)):>12} {route:>16} " + " ".join(f"{v:>9.1f}" for r in rounds for v in r) + f" {ratio:>17.3f}")
        print(lines[-1], flush=True)
    lines.append("")
    lines.append("the 2-D yardstick of the same run: k10_sweep, periodic 4096 x 4096, T = T_c(q), three rounds, us per sweep")
    for q in (3, 8):
        us = [k10_2d_sweep_us(4096, q, 10) for _ in range(3)]
        res["k10_2d"].append({"L": 4096, "q": q, "us_per_sweep": us})
        lines.append(f"{'k10_sweep':>12} {4096:>5} q={q} " + " ".join(f"{v:>8.1f}" for v in us))
        print(lines[-1], flush=True)
    if not a.no_resources:
        res["resources"] = kernel_resources()
        lines.append("")
        lines.append("kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)")
        lines.append(f"{'kernel':>21} {'VGPRs':>6} {'SGPRs':>6} {'LDS B (static)':>14} {'scratch B/lane':>14}")
        for k, v in sorted(res["resources"].items()):
            lines.append(f"{k:>21} {v.get('vgprs', -1):>6} {v.get('sgprs', -1):>6} {v.get('lds', -1):>14} {v.get('scratch', -1):>14}")
            print(lines[-1], flush=True)
        lines.append("(dynamic LDS on top: k10_3d_sw_small 5 B a site, k10_3d_sw_local 5 B a tile site = 20480 B at 8 x 16 x 32, 81920 B at 16 x 32 x 32)")
    with open(os.path.join(a.out, "potts3d_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(a.out, "potts3d_time.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

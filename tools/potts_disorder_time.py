"""K12, Potts lattices with stored couplings: site updates per second of k12_sweep (4096^2 and 256^3, q = 3 and 8, with and without a
site field) beside k10_sweep on the same shapes and k7_sweep / k8_sweep on constant arrays, k12_small at 64^2 and 16^3, and a
Swendsen-Wang step on bimodal couplings J in {1, 2} beside K10's step, all in one run; the registers, LDS and scratch of every K12
kernel and of every k10_* kernel (the latter also from a checkout of the parent commit, if one is given) from the compiler's resource
remarks; and the static instruction counts of the k12_sweep instantiations.

    python tools/potts_disorder_time.py [--out DIR] [--no-resources] [--baseline ROOT] [--commit LABEL] [--quick]

Device events after warm-up, medians of 5; one process.  Writes DIR/potts_disorder_time.txt (default DIR: profiles/)."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))
from tsu import _hip  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only"]
ROUNDS = 5


def _median_ms(ctx, fn):
    """fn(k) runs round k; the median of ROUNDS device-event times."""
    ms = []
    for k in range(ROUNDS):
        ctx.synchronize()
        ctx.timer_begin()
        fn(k)
        ms.append(ctx.timer_end())
    return float(np.median(ms)), ms


def _constant(shape, per, J):
    out = []
    for k in range(len(shape)):
        a = np.full(shape, J, np.float32)
        axis = len(shape) - 1 - k
        if not per:
            a[(slice(None),) * axis + (-1,)] = 0.0
        out.append(a)
    return out


def _disorder(shape, q, field, rng, kind):
    if kind == "gaussian":
        J = [rng.standard_normal(size=shape, dtype=np.float32) for _ in shape]
    else:  # bimodal {1, 2}
        J = [(1.0 + (rng.random(size=shape, dtype=np.float32) < 0.5)).astype(np.float32) for _ in shape]
    h = rng.standard_normal(size=(q,) + tuple(shape), dtype=np.float32) if field else None
    return J, h


def _k12(shape, q, J, h, spins):
    lat = _hip.PottsDisorderLattice(shape, q, True)
    lat.set_disorder(J[0], J[1], J[2] if len(J) == 3 else None, h)
    lat.set_spins(spins)
    return lat


def _k10(shape, q, spins):
    lat = _hip.PottsLattice(shape[0], shape[1], q, True) if len(shape) == 2 else _hip.PottsLattice3D(*shape, q, True)
    lat.set_spins(spins)
    return lat


def heat_bath_rates(shape, q, n, say):
    """k12_sweep with Gaussian couplings with and without a Gaussian field, then k10_sweep, on one random start at T = 1.0."""
    rng = np.random.default_rng(1)
    sites = int(np.prod(shape))
    spins = rng.integers(0, q, size=shape).astype(np.int8)
    name = "x".join(map(str, shape))
    out = {}
    for field in (False, True):
        J, h = _disorder(shape, q, field, rng, "gaussian")
        lat = _k12(shape, q, J, h, spins)
        del J, h
        lat.sweep(1.0, 2, 7, 0)
        ms, all_ms = _median_ms(lat.ctx, lambda k: lat.sweep(1.0, n, 7, 2 + k * n))
        route = lat.route()
        lat.close()
        rate = sites * n / (ms * 1e-3)
        dim = len(shape)
        model_bytes = 8 * dim + 4 + (8 * q if field else 0)  # 2 planes a bond axis read in both half-sweeps, q field planes, spins
        say(f"{name:>12} {q:>2} {'k12, field' if field else 'k12, no field':>16} {route:>10} {n:>3} {ms:>9.3f} {rate:>10.3e} "
            f"{rate * model_bytes / 1e12:>6.2f}  " + " ".join(f"{v:.3f}" for v in all_ms))
        out[field] = rate
    lat = _k10(shape, q, spins)
    lat.sweep(1.0, 2, 7, 0)
    ms, all_ms = _median_ms(lat.ctx, lambda k: lat.sweep(1.0, n, 7, 2 + k * n))
    route = lat.route()
    lat.close()
    say(f"{name:>12} {q:>2} {'k10':>16} {route:>10} {n:>3} {ms:>9.3f} {sites * n / (ms * 1e-3):>10.3e} {'':>6}  " + " ".join(f"{v:.3f}" for v in all_ms))
    return out


def ising_rates(n, say):
    """k7_sweep (4096^2) and k8_sweep (256^3) on constant arrays J = 1, h = 0 at T = 2.0: the two-valued lattices with stored bonds."""
    rng = np.random.default_rng(1)
    l2 = _hip.Lattice(4096, 4096, True)
    l2.randomize(3)
    one = np.ones((4096, 4096), np.float32)
    l2.set_disorder(one, one, 0 * one)
    l2.disorder_sweep(2.0, 2, 7, 0)
    ms, all_ms = _median_ms(l2.ctx, lambda k: l2.disorder_sweep(2.0, n, 7, 2 + k * n))
    l2.close()
    say(f"{'4096x4096':>12} {2:>2} {'k7 (Ising)':>16} {'k7_sweep':>10} {n:>3} {ms:>9.3f} {4096 * 4096 * n / (ms * 1e-3):>10.3e} {'':>6}  "
        + " ".join(f"{v:.3f}" for v in all_ms))
    l3 = _hip.Lattice3D(256, 256, 256, (True, True, True))
    l3.randomize(3)
    one = np.ones((256, 256, 256), np.float32)
    l3.set_disorder(one, one, one, 0 * one)
    l3.sweep(2.0, 2, 7, 0)
    ms, all_ms = _median_ms(l3.ctx, lambda k: l3.sweep(2.0, n, 7, 2 + k * n))
    l3.close()
    say(f"{'256x256x256':>12} {2:>2} {'k8 (Ising)':>16} {'k8_sweep':>10} {n:>3} {ms:>9.3f} {256 ** 3 * n / (ms * 1e-3):>10.3e} {'':>6}  "
        + " ".join(f"{v:.3f}" for v in all_ms))
    del rng


def small_rates(shape, q, n, say):
    rng = np.random.default_rng(1)
    spins = rng.integers(0, q, size=shape).astype(np.int8)
    J, h = _disorder(shape, q, True, rng, "gaussian")
    name = "x".join(map(str, shape))
    for label, lat in (("k12, field", _k12(shape, q, J, h, spins)), ("k10", _k10(shape, q, spins))):
        lat.sweep(1.0, 2, 7, 0)
        ms, all_ms = _median_ms(lat.ctx, lambda k: lat.sweep(1.0, n, 7, 2 + k * n))
        say(f"{name:>12} {q:>2} {label:>16} {lat.route():>10} {n:>3} {ms:>9.3f} {int(np.prod(shape)) * n / (ms * 1e-3):>10.3e} {'':>6}  "
            + " ".join(f"{v:.3f}" for v in all_ms))
        lat.close()


def cluster_rates(shape, q, T, n, say):
    """A Swendsen-Wang step on bimodal couplings J in {1, 2} (k12) and on J = 1 (k10) from the same random start, n steps a round."""
    rng = np.random.default_rng(1)
    spins = rng.integers(0, q, size=shape).astype(np.int8)
    J, _ = _disorder(shape, q, False, rng, "bimodal")
    name = "x".join(map(str, shape))
    for label, lat in (("k12, J in {1,2}", _k12(shape, q, J, None, spins)), ("k10, J = 1", _k10(shape, q, spins))):
        lat.cluster_sweep(T, 2, 7, 0)
        ms, all_ms = _median_ms(lat.ctx, lambda k: lat.cluster_sweep(T, n, 7, 2 + k * n))
        lat.get_spins()  # reports a cap that expired
        say(f"{name:>12} {q:>2} {label:>16} {lat.route(_hip.POTTS_SWENDSEN_WANG):>12} {T:>6.3f} {n:>3} {ms / n:>9.3f} {int(np.prod(shape)) * n / (ms * 1e-3):>10.3e}  "
            + " ".join(f"{v / n:.3f}" for v in all_ms))
        lat.close()


# ---------------------------------------------------------------- the compiler's view
def _demangle(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not filt:
        return {n: n for n in names}
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    clean = [re.sub(r"\(.*$", "", re.sub(r"^void |\(anonymous namespace\)::", "", s)) for s in out]
    return dict(zip(names, clean))


def kernel_resources(csrc, source, pattern):
    """{kernel: (VGPRs, AGPRs, SGPRs, scratch B/lane, LDS B, waves/SIMD)} of the kernels of csrc/source whose name matches."""
    r = subprocess.run([HIPCC, *FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, source), "-o", os.devnull],
                       capture_output=True, text=True, cwd=csrc)
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    names = _demangle([b.split()[0] for b in blocks])
    out = {}
    for b in blocks:
        name = names[b.split()[0]]
        if not re.search(pattern, name):
            continue
        vals = []
        for key in (r" VGPRs", r"AGPRs", r"TotalSGPRs", r"ScratchSize \[bytes/lane\]", r"LDS Size \[bytes/block\]", r"Occupancy \[waves/SIMD\]"):
            m = re.search(key + r": (\d+)", b)
            vals.append(int(m.group(1)) if m else -1)
        out[name] = tuple(vals)
    return out


def instruction_counts(csrc):
    """Static instruction counts of the k12_sweep instantiations from the device assembly: all, float64 VALU, global loads."""
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "pd.s")
        subprocess.run([HIPCC, *FLAGS, "-S", os.path.join(csrc, "potts_disorder.hip"), "-o", asm], check=True, capture_output=True, cwd=csrc)
        text = open(asm).read()
    out = {}
    starts = [(m.start(), m.group(1)) for m in re.finditer(r"^(_Z\w*k12_sweep\w*):", text, flags=re.M)]
    names = _demangle([n for _, n in starts])
    for pos, name in starts:
        body = text[pos:text.index("s_endpgm", pos)]
        ins = [ln.split()[0] for ln in body.splitlines()[1:] if ln.startswith("\t") and ln.strip() and not ln.strip().startswith((".", ";"))]
        out[names[name]] = (len(ins), sum(1 for i in ins if i.startswith("v_") and "f64" in i), sum(1 for i in ins if i.startswith("global_load")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--baseline", default=None, help="the root of a checkout of the parent commit: its k10_* kernels are compiled as well")
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

    big2, big3 = ((512, 512), (64, 64, 64)) if a.quick else ((4096, 4096), (256, 256, 256))
    say("heat-bath sweeps, periodic lattices, random start, T = 1.0, Gaussian couplings (and field); device events after 2 warm-up sweeps,")
    say(f"the median of {ROUNDS} rounds of n sweeps; TB/s: updates/s times the model's bytes per site and sweep, (8 DIM + 8 q [field] + 4) B")
    say(f"{'lattice':>12} {'q':>2} {'kernel':>16} {'route':>10} {'n':>3} {'ms/round':>9} {'updates/s':>10} {'TB/s':>6}  rounds (ms)")
    for shape in (big2, big3):
        for q in (3, 8):
            heat_bath_rates(shape, q, 5, say)
    if not a.quick:
        ising_rates(5, say)
    say()
    say("one workgroup (k12_small / k10_small), all sweeps of a round in one launch")
    say(f"{'lattice':>12} {'q':>2} {'kernel':>16} {'route':>10} {'n':>3} {'ms/round':>9} {'updates/s':>10} {'':>6}  rounds (ms)")
    for shape in ((64, 64), (16, 16, 16)):
        for q in (3, 8):
            small_rates(shape, q, 200, say)
    say()
    say("Swendsen-Wang steps, periodic, random start, T near the pure model's T_c (2-D: 1 / ln(1 + sqrt q); 3-D q = 3: 1.8163); ms per step")
    say(f"{'lattice':>12} {'q':>2} {'kernel':>16} {'route':>12} {'T':>6} {'n':>3} {'ms/step':>9} {'updates/s':>10}  rounds (ms/step)")
    for shape, q, T in ((big2, 3, 1.0 / np.log(1.0 + np.sqrt(3.0))), (big2, 8, 1.0 / np.log(1.0 + np.sqrt(8.0))), (big3, 3, 1.8163)):
        cluster_rates(shape, q, float(T), 5, say)
    if not a.no_resources:
        csrc = os.path.join(ROOT, "tsu-emulator_amd", "csrc")
        say()
        say("kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): K12's kernels (the one-workgroup cluster kernels add")
        say("5 B of dynamic LDS a site, the tile pass 5 B a tile site)")
        head = f"{'kernel':>34} {'VGPRs':>6} {'AGPRs':>6} {'SGPRs':>6} {'scratch B/lane':>14} {'LDS B':>7} {'waves/SIMD':>10}"
        say(head)
        for k, v in kernel_resources(csrc, "potts_disorder.hip", r"^k12_").items():
            say(f"{k:>34} " + " ".join(f"{x:>{w}}" for x, w in zip(v, (6, 6, 6, 14, 7, 10))))
        say()
        say("static instruction counts of k12_sweep (device assembly): all, float64 VALU, global loads")
        for k, v in instruction_counts(csrc).items():
            say(f"{k:>34} {v[0]:>6} {v[1]:>6} {v[2]:>6}")
        say()
        say("K10's kernels as the compiler leaves them now" + (" and in the parent commit" if a.baseline else ""))
        say(head + ("   parent: the same columns" if a.baseline else ""))
        same = True
        for src in ("potts2d.hip", "potts3d.hip"):
            now = kernel_resources(csrc, src, r"^k10_")
            was = kernel_resources(os.path.join(a.baseline, "tsu-emulator_amd", "csrc"), src, r"^k10_") if a.baseline else {}
            for k, v in now.items():
                tail = ""
                if a.baseline:
                    tail = "   " + " ".join(str(x) for x in was.get(k, ())) + ("" if was.get(k) == v else "   <-- differs")
                    same = same and was.get(k) == v
                say(f"{k:>34} " + " ".join(f"{x:>{w}}" for x, w in zip(v, (6, 6, 6, 14, 7, 10))) + tail)
        if a.baseline:
            say("every k10_* kernel: " + ("no change" if same else "CHANGED"))
    with open(os.path.join(a.out, "potts_disorder_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

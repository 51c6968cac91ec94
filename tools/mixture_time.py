"""K3 Gaussian mixtures: (a) the reference's multimodal demo through the Python API, (b) kernel throughput of k3_mixture_*.

usage:
  python tools/mixture_time.py [--out FILE.json]            times (a) and (b) on the GPU, prints a table, writes the numbers
  python tools/mixture_time.py --kernels-only               (b) alone, one timed call per case (for a rocprofv3 --pmc run)
  python tools/mixture_time.py --report FILE.json PMC.csv   issue-ceiling fractions of (b) from the times and a counter run
                                                            (rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES -- ... --kernels-only);
                                                            the recorded pair: profiles/mixture_time.json,
                                                            profiles/mixture_pmc_counter_collection.csv

(a) The demo (tsu/demos.py:89-105): 3 temperatures x 166 samples x 10-D, 100 burn-in + 300 steps, sample_from_energy on the demo's
bound energy method (recognised as a mixture); the reference's published time for this workload is 28.93 s (tsu/hardware.py:185).
(b) 1000 fused steps per call, timed with tsu_timer_* (device events): element-steps/s.  The VALU issue ceiling: one wave's
instruction stream on one SIMD costs 4 cycles per VALU instruction and 8 per transcendental (v_exp / v_log / v_sqrt / v_sin /
v_cos / v_rcp), 256 CUs x 4 SIMDs at 2.4 GHz; VALU per wave-step from SQ_INSTS_VALU / SQ_WAVES / steps (counters), transcendentals
per wave-step from the kernel (K + ceil(K/8) exp2 and one rcp per chain, 8 per quad of Box-Muller; one exp2 per component, one
for eps, one rcp per workgroup-step of the workgroup kernel, counted per wave)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

REF_DEMO_S = 28.93
CLOCK_HZ = 2.4e9
SIMDS = 256 * 4
STEPS = 1000
CASES = [  # (name, chains, dim, K)
    ("lane d16 K4", 65536, 16, 4),
    ("lane d64 K16", 65536, 64, 16),
    ("wg d4096 K8", 256, 4096, 8),
]


class _ModeMixture:
    """An object of the demo distribution's shape, as recognition sees it: ``mode_centers`` (K, d), ``mode_weights`` (K,) and a bound
    energy E(x) = -log(sum_i w_i exp(-||x - mu_i||^2 / 2) + 1e-10), written here from that formula."""

    def __init__(self, centers, weights):
        self.mode_centers = np.asarray(centers, dtype=np.float64)
        self.mode_weights = np.asarray(weights, dtype=np.float64)

    def energy(self, x):
        d2 = np.sum((np.atleast_1d(x)[None, :] - self.mode_centers) ** 2, axis=1)
        return float(-np.log(np.exp(-0.5 * d2) @ self.mode_weights + 1e-10))


def demo(repeats=5):
    """The demo's workload (its published 28.93 s): 10-D, three modes (centres N(0, 9 I), weights 0.3 / 0.5 / 0.2), at T = 0.5, 1
    and 2 one sample_from_energy call of 166 restarts, 100 burn-in and 300 steps each, started near 0."""
    from tsu.core import ThermalSamplingUnit, TSUConfig
    rng = np.random.default_rng(0)
    target = _ModeMixture(3.0 * rng.standard_normal((3, 10)), [0.3, 0.5, 0.2])
    starts = {T: 0.5 * rng.standard_normal(10) for T in (0.5, 1.0, 2.0)}

    def one_pass():
        times, n = [], 0
        for T, x0 in starts.items():
            t0 = time.perf_counter()
            unit = ThermalSamplingUnit(TSUConfig(temperature=T, n_burnin=100, n_steps=300), seed=int(10 * T))
            n += unit.sample_from_energy(target.energy, x0, n_samples=166).shape[0]
            times.append(time.perf_counter() - t0)
        return times, n

    one_pass()  # (first call: code objects, context)
    runs = [one_pass() for _ in range(repeats)]
    per, n = min(runs, key=lambda r: sum(r[0]))
    tot = sum(per)
    return {"total_s": tot, "per_call_s": per, "samples": [n, 10], "reference_s": REF_DEMO_S, "speedup": REF_DEMO_S / tot}


def kernels(reps=3):
    from tsu import _hip
    ctx = _hip.Context.default()
    res = []
    for name, chains, dim, K in CASES:
        rng = np.random.default_rng(dim + K)
        c = rng.standard_normal((K, dim)) * (3.0 / np.sqrt(dim))
        lc = _hip.LangevinChains(chains, dim, ctx=ctx)
        lc.set_mixture(c, rng.uniform(0.2, 1.0, K), np.linspace(0.8, 1.2, K), 1e-10)
        lc.set_state((c[np.arange(chains) % K] + 0.1 * rng.standard_normal((chains, dim))).astype(np.float32))
        lc.step(20, 0.01, 1.0, 1.0, 5)
        ctx.synchronize()
        best = 1e30
        for r in range(reps):
            ctx.timer_begin()
            lc.step(STEPS, 0.01, 1.0, 1.0, 5, step0=20 + r * STEPS)
            best = min(best, ctx.timer_end())
        x = lc.get_state()
        lc.close()
        res.append({"case": name, "chains": chains, "dim": dim, "K": K, "steps": STEPS, "ms": best,
                    "element_steps_per_s": chains * dim * STEPS / (best * 1e-3), "finite": bool(np.all(np.isfinite(x)))})
    return res


def _trans_per_wave_step(chains, dim, K):
    quads = (dim + 3) // 4
    if dim <= 64:  # 64 chains per wave, each lane all of its chain
        return K + (K + 7) // 8 + 1 + 8 * quads
    t = min(1024, ((quads + 3) // 4 + 63) // 64 * 64)  # the workgroup kernel's shape (k3m_wg_shape)
    qpt = 1
    while qpt * t < quads:
        qpt *= 2
    return 2 + 1 + 8 * qpt  # (lane i < K: one exp2 each and the eps term, one rcp: one instruction per wave)


def report(times_path, pmc_path):
    import csv
    with open(times_path) as f:
        times = json.load(f)
    rows = list(csv.DictReader(open(pmc_path)))
    by_kernel = {}
    for r in rows:
        nm = r.get("Kernel_Name", "")
        if "k3_mixture" not in nm:
            continue
        key = (nm, r.get("Dispatch_Id", r.get("Correlation_Id", "")))
        by_kernel.setdefault(key, {})[r["Counter_Name"]] = by_kernel.get(key, {}).get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    disp = [v for k, v in sorted(by_kernel.items(), key=lambda kv: int(kv[0][1]) if str(kv[0][1]).isdigit() else 0)]
    # dispatches in order: per case one warm-up call (20 steps) then the timed call (STEPS) in --kernels-only
    out = []
    for i, t in enumerate(times["kernels"]):
        cnt = disp[2 * i + 1]
        valu_ws = cnt["SQ_INSTS_VALU"] / cnt["SQ_WAVES"] / STEPS
        tr = _trans_per_wave_step(t["chains"], t["dim"], t["K"])
        cyc = 4 * (valu_ws - tr) + 8 * tr
        waves = cnt["SQ_WAVES"]
        ceiling_s = waves * STEPS * cyc / (SIMDS * CLOCK_HZ)
        frac = ceiling_s / (t["ms"] * 1e-3)
        out.append(dict(t, valu_per_wave_step=valu_ws, trans_per_wave_step=tr, issue_cycles_per_wave_step=cyc,
                        ceiling_ms=ceiling_s * 1e3, fraction_of_issue_ceiling=frac))
        print(f"{t['case']:>14}: {t['element_steps_per_s']:.3e} element-steps/s; {valu_ws:.1f} VALU ({tr} transcendental) per wave-step "
              f"= {cyc:.0f} issue cycles; ceiling {ceiling_s * 1e3:.2f} ms vs {t['ms']:.2f} ms measured = {frac:.2f} of the VALU issue ceiling")
    return out


def main():
    args = sys.argv[1:]
    if args[:1] == ["--report"]:
        res = report(args[1], args[2])
        if len(args) > 3:
            with open(args[3], "w") as f:
                json.dump(res, f, indent=1)
        return
    if args[:1] == ["--kernels-only"]:
        kernels(reps=1)
        return
    out = args[args.index("--out") + 1] if "--out" in args else None
    from tsu import _hip
    print("device:", _hip.Context.default().device_info())
    dm = demo()
    print(f"demo (3 temperatures x 166 samples x 10-D x 400 steps) through sample_from_energy: {dm['total_s'] * 1e3:.1f} ms in all "
          f"({', '.join(f'{p * 1e3:.1f}' for p in dm['per_call_s'])} ms per call); the reference: {REF_DEMO_S} s "
          f"({dm['speedup']:.0f}x)")
    ks = kernels()
    for k in ks:
        print(f"{k['case']:>14}: {k['chains']} chains x d {k['dim']} x K {k['K']}, {STEPS} fused steps: {k['ms']:.2f} ms = "
              f"{k['element_steps_per_s']:.3e} element-steps/s")
    if out:
        with open(out, "w") as f:
            json.dump({"demo": dm, "kernels": ks}, f, indent=1)


if __name__ == "__main__":
    main()

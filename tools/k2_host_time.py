"""Host time per K2 call between two builds of the library on ONE box: loops of one-sweep calls (annealing, tempering), where the
launch envelope and the kept-field bookkeeping are what a call costs beside a 30-100 us kernel.  Each build runs in a fresh child
process (TSU_HIP_LIB), the two alternating, one process at a time; a row passes when the new build's median does not exceed the
parent's by more than the parent's own spread (largest minus smallest of its repetitions).
usage: python tools/k2_host_time.py parent.so new.so [--reps 5] [--out table.txt]      child: python tools/k2_host_time.py --child"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _system(hip, ctx, n, f64=False):
    import numpy as np
    rng = np.random.default_rng(n)
    G = rng.standard_normal((n, n))
    J = (G + G.T) / 2 / np.sqrt(n)
    np.fill_diagonal(J, 0.0)
    d = hip.DenseSystem(J if f64 else J.astype(np.float32), None, hip.DTYPE_F64 if f64 else hip.DTYPE_F32, ctx=ctx)
    d.set_state(rng.integers(0, 2, size=n).astype(np.int8))
    return d


def child():
    """One JSON line: microseconds per call (wall clock of a window of calls, one synchronise at its end, after warm-up calls of the
    same shape), and the benchmark's own three K2 figures in ms."""
    sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))
    sys.path.insert(0, ROOT)
    import numpy as np
    from tsu import _hip as hip
    ctx = hip.Context(0)
    rows = {}

    def loop(d, calls, warm=20):
        for i in range(warm):
            d.sweep(1.0, 1, seed=1, sweep0=i)
        ctx.synchronize()
        t0 = time.perf_counter()
        for i in range(calls):
            d.sweep(1.0, 1, seed=1, sweep0=warm + i)
        ctx.synchronize()
        return (time.perf_counter() - t0) / calls * 1e6

    for name, n, f64, calls, which in (("sweep(T,1) n=2048 f32 k2_own", 2048, False, 200, 0), ("sweep(T,1) n=4096 f32 k2_own", 4096, False, 200, 0),
                                       ("sweep(T,1) n=1024 f32 k2_pipe", 1024, False, 200, 1), ("sweep(T,1) n=2051 f64 k2_coop", 2051, True, 50, None)):
        d = _system(hip, ctx, n, f64)
        rows[name + " [us/call]"] = loop(d, calls)
        counts = d.launch_counts()
        assert counts == tuple(calls + 20 if q == which else 0 for q in range(2)), (name, counts)  # (the kernel the row names)
        d.close()
    # a tempering round: four replicas advance one sweep together, then the ladder asks for their energies
    n, R = 2304, 4
    d = _system(hip, ctx, n)
    sts = np.array([np.random.default_rng(100 + r).integers(0, 2, size=n) for r in range(R)], dtype=np.int8)
    for k in range(10):
        sts = d.sweep_replicas(sts, [1.0, 1.3, 1.7, 2.2], 1, list(range(R)), [k] * R)
        d.energies(sts)
    ctx.synchronize()
    t0 = time.perf_counter()
    for k in range(100):
        sts = d.sweep_replicas(sts, [1.0, 1.3, 1.7, 2.2], 1, list(range(R)), [10 + k] * R)
        d.energies(sts)
    ctx.synchronize()
    rows["sweep_replicas(R=4, 1 sweep) + energies n=2304 [us/round]"] = (time.perf_counter() - t0) / 100 * 1e6
    d.sample(1.0, 0, 1, 64, seed=3, sweep0=0)
    ctx.synchronize()
    t0 = time.perf_counter()
    d.sample(1.0, 0, 1, 64, seed=3, sweep0=64)
    ctx.synchronize()
    rows["sample(64 recorded states) n=2304 [us/call]"] = (time.perf_counter() - t0) * 1e6
    d.close()
    import bench
    b = bench.time_dense(hip, ctx, {})
    rows["bench N=16384 natural order [ms/sweep]"] = b["ms_per_sweep"]
    rows["bench N=16384 caller's order [ms/sweep]"] = b["random_order"]["ms_per_sweep"]
    rows["bench N=16384 eight replicas [ms/sweep]"] = b["eight_replicas"]["ms_per_all_replica_sweep"]
    print("K2HOST " + json.dumps(rows), flush=True)


def main(argv):
    libs = [os.path.abspath(a) for a in argv[:2]]
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 5
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    got = [[], []]
    for rep in range(reps):
        for which, lib in enumerate(libs):  # parent, new, parent, new, ...: one process at a time
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, TSU_HIP_LIB=lib), capture_output=True,
                               text=True, timeout=300)
            line = [x for x in r.stdout.splitlines() if x.startswith("K2HOST ")]
            if r.returncode or not line:  # nothing more runs on the GPU after a child that failed
                print(r.stdout[-2000:], r.stderr[-4000:])
                return 1
            got[which].append(json.loads(line[0][7:]))
            print(f"rep {rep} {'parent' if which == 0 else 'new'} done", flush=True)
    text = [f"K2 host time, parent against new build, {reps} alternating child processes each (tools/k2_host_time.py)",
            f"{'row':62s} {'parent median':>14s} {'parent min..max':>22s} {'new median':>12s} {'new min..max':>22s}  verdict"]
    failed = 0
    for name in got[0][0]:
        p, q = [g[name] for g in got[0]], [g[name] for g in got[1]]
        ok = statistics.median(q) <= statistics.median(p) + (max(p) - min(p))
        failed += not ok
        text.append(f"{name:62s} {statistics.median(p):14.3f} {min(p):10.3f} ..{max(p):10.3f} {statistics.median(q):12.3f} {min(q):10.3f} ..{max(q):10.3f}  "
                    f"{'pass' if ok else 'FAIL'}")
    text.append(f"{failed} rows failed")
    print("\n".join(text))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(text) + "\n")
    return 0


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:
        child()
    else:
        sys.exit(main(sys.argv[1:]))

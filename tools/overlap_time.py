"""Overlaps of walker pairs: the link pass against the spin-overlap pass on the same planes, and what recording the overlaps adds to
a population step and to a ladder round.  One process per shape (a parent that starts a fresh child per case and collects its JSON
line); periodic lattices, Gaussian J.

  kernels   per case, a child under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters) makes a few calls that launch
            both passes on the same planes; from its kernel stats: the mean time of the link pass (link_pass / pt_link) and of the
            spin-overlap pass (k7_overlap / k8_overlap / pt_overlap), their ratio, and bytes/s counting the 2 B per site both must
            read at least (the link pass's second read of the layer neighbour is not counted: the figure is what a user gets per
            site, not the traffic).
            Cases: pair2d:8192  pair3d:256  ladder2d:4096x16  ladder3d:256x8  pop2d:64x65535  pop3d:16x8192
  share     per case, device events around recorded calls that end in a synchronise, switches off and on alternating in one
            process, theta = 10, REPS timed calls each after a warm-up: the medians, their spread (max - min over the median) and the
            added share (on - off) / off.  Populations: overlap on, and overlap + correlation on.  Ladders (two ladders; off already
            records q): link_overlap on.
            Cases: pop2d:64x4096  pop2d:64x65535  pop3d:16x8192  pop2d:4096x64  ladder2d:4096x16  ladder3d:256x8

    python tools/overlap_time.py [--out DIR] [--kernels CASES] [--share CASES]      ('' skips a part)

Writes DIR/overlap_time.txt and DIR/overlap_time.json (default DIR: profiles/)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))

HBM_PEAK = 8.0e12  # bytes/s, MI355X nominal
THETA = 10
REPS = 5
KERNEL_CASES = "pair2d:8192,pair3d:256,ladder2d:4096x16,ladder3d:256x8,pop2d:64x65535,pop3d:16x8192"
SHARE_CASES = "pop2d:64x4096,pop2d:64x65535,pop3d:16x8192,pop2d:4096x64,ladder2d:4096x16,ladder3d:256x8"


def parse(case):
    kind, rest = case.split(":")
    dim = int(kind[-2])
    nums = [int(x) for x in rest.split("x")]
    return kind[:-2], dim, nums[0], (nums[1] if len(nums) > 1 else 2)


def disorder(dim, L):
    rng = np.random.default_rng(1)
    return tuple(rng.normal(size=(L,) * dim).astype(np.float32) for _ in range(dim))


def make(kind, dim, L, n, theta, **switches):
    from tsu.models import ising
    dis = disorder(dim, L)
    if kind == "pop":
        cls = ising.PopulationAnnealing if dim == 2 else ising.PopulationAnnealing3D
        db = 0.5 / np.sqrt(dim * L ** dim)
        return cls((L,) * dim, n, betas=0.5 + db * np.arange(4097), couplings=dis, seed=3, sweeps_per_step=theta, **switches)
    cls = ising.LatticeTempering if dim == 2 else ising.LatticeTempering3D
    return cls((L,) * dim, np.linspace(2.0, 1.0, n), couplings=dis, seed=3, ladders=2, **switches)


# ---------------------------------------------------------------- children
def child_kernels(case):
    """The calls a kernel trace is taken of: both passes on the same planes, five launches each after one warm-up."""
    from tsu import _hip
    kind, dim, L, n = parse(case)
    if kind == "pair":
        cls = _hip.Lattice if dim == 2 else _hip.Lattice3D
        a, b = cls(*((L,) * dim), True), cls(*((L,) * dim), True)
        a.randomize(1)
        b.randomize(2)
        for _ in range(6):
            a.overlap(b)
            a.link_overlap(b)
    elif kind == "pop":
        pa = make(kind, dim, L, n, 1, overlap=True)
        pa._pa.run(5, 1, True, True)
        pa._pa.history()
    else:
        pt = make(kind, dim, L, n, 1, link_overlap=True)
        pt._pt.run(6, 1, True, True)
        pt._pt.history()
    print(json.dumps(dict(case=case)))


def child_share(case):
    from tsu import _hip
    kind, dim, L, n = parse(case)
    ctx = _hip.Context.default()
    N = L ** dim
    variants = ([("off", {}), ("overlap", dict(overlap=True)), ("overlap+correlation", dict(overlap=True, correlation=True))]
                if kind == "pop" else [("off", {}), ("link_overlap", dict(link_overlap=True))])
    per = max(1, min(8, int(4e9 / (N * n * (1 if kind == "pop" else 2) * THETA))))
    handles = [(name, make(kind, dim, L, n, THETA, **sw)) for name, sw in variants]

    def call(h):
        if kind == "pop":
            h._pa.run(per, THETA, True, True)
        else:
            h._pt.run(per, THETA, True, True)
    times = {name: [] for name, _ in variants}
    for name, h in handles:  # warm-up of every shape the timed window uses
        call(h)
    ctx.synchronize()
    for _ in range(REPS):  # alternating
        for name, h in handles:
            ctx.timer_begin()
            call(h)
            times[name].append(ctx.timer_end() / per)
    print(json.dumps(dict(case=case, calls_of=per, ms={k: v for k, v in times.items()})))


# ---------------------------------------------------------------- parent
def run_child(args, prefix=()):
    r = subprocess.run(list(prefix) + [sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"{args}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def kernel_stats(case):
    with tempfile.TemporaryDirectory() as d:
        run_child(["--child-kernels", case], prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--"])
        found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            raise RuntimeError(f"{case}: rocprofv3 wrote no kernel stats")
        with open(found[0]) as f:
            return list(csv.DictReader(f))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--kernels", default=KERNEL_CASES)
    ap.add_argument("--share", default=SHARE_CASES)
    ap.add_argument("--child-kernels")
    ap.add_argument("--child-share")
    a = ap.parse_args()
    if a.child_kernels:
        return child_kernels(a.child_kernels)
    if a.child_share:
        return child_share(a.child_share)
    lines, out = [], dict(theta=THETA, reps=REPS, hbm_peak=HBM_PEAK, kernels=[], share=[])
    for case in [c for c in a.kernels.split(",") if c]:
        kind, dim, L, n = parse(case)
        pairs = 1 if kind == "pair" else (n // 2 if kind == "pop" else n)
        rows = kernel_stats(case)

        def mean_ns(names):
            hit = [r for r in rows if any(k + "(" in r["Name"] for k in names)]
            calls = sum(int(r["Calls"]) for r in hit)
            return sum(float(r["TotalDurationNs"]) for r in hit) / calls if calls else float("nan")
        link, spin = mean_ns(["link_pass", "pt_link"]), mean_ns(["k7_overlap", "k8_overlap", "pt_overlap"])
        nbytes = 2.0 * L ** dim * pairs
        row = dict(case=case, pairs=pairs, link_us=link / 1e3, overlap_us=spin / 1e3, ratio=link / spin, bytes=nbytes,
                   link_bytes_per_s=nbytes / (link * 1e-9), overlap_bytes_per_s=nbytes / (spin * 1e-9))
        out["kernels"].append(row)
        lines.append(f"kernels {case}: {pairs} pair(s) of {L}^{dim}: link pass {link / 1e3:.1f} us, spin-overlap pass {spin / 1e3:.1f} us, ratio "
                     f"{link / spin:.2f}; at 2 B per site {row['link_bytes_per_s'] / 1e12:.2f} TB/s against {row['overlap_bytes_per_s'] / 1e12:.2f} "
                     f"TB/s ({row['link_bytes_per_s'] / HBM_PEAK:.2f} and {row['overlap_bytes_per_s'] / HBM_PEAK:.2f} of HBM peak)")
        print(lines[-1], flush=True)
    for case in [c for c in a.share.split(",") if c]:
        r = run_child(["--child-share", case])
        med = {k: float(np.median(v)) for k, v in r["ms"].items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in r["ms"].items()}
        row = dict(case=case, calls_of=r["calls_of"], median_ms=med, spread=spread,
                   added={k: (med[k] - med["off"]) / med["off"] for k in med if k != "off"})
        out["share"].append(row)
        what = "step" if case.startswith("pop") else "round"
        lines.append(f"share {case}: recorded {what}, theta = {THETA}, median of {REPS} calls of {r['calls_of']}: off {med['off'] * 1e3:.1f} us "
                     f"(spread {spread['off']:.3f})" + "".join(f"; {k} {med[k] * 1e3:.1f} us (spread {spread[k]:.3f}): {row['added'][k]:+.4f}"
                                                              for k in med if k != "off"))
        print(lines[-1], flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "overlap_time.json"), "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.join(a.out, "overlap_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

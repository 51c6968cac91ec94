"""K8 heat-bath sweeps of 3-D disordered lattices: us per sweep at 64^3, 128^3 and 256^3 (periodic, Gaussian bonds + fields,
T = 2.0) at 1, 16 and 100 sweeps per call (device events around calls that end in a synchronise, every shape warmed up, medians
of 5), with the bytes a sweep of K8 moves and the fraction of HBM peak they reach; and in the same run K7 at 4096^2 (the site
count of 256^3) and the K5 CSR gather route (the general-graph kernel) on the same 256^3 couplings, the route a 3-D lattice
had before K8.

    python tools/lattice3d_time.py [--out DIR] [--sizes 64,128,256] [--no-k5] [--no-k7]
    python tools/lattice3d_time.py --shapes [--out DIR]

Writes DIR/lattice3d_time.txt and DIR/lattice3d_time.json (default DIR: profiles/).  --shapes instead times lattices of 2^24
sites of other shapes (wide rows, thin rows, one layer without z neighbours) at 16 sweeps per call: DIR/lattice3d_shapes.txt."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsu-emulator_amd"))
from tsu import _hip  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X nominal
T = 2.0


def disorder(shape, seed=1):
    rng = np.random.default_rng(seed)
    return tuple(rng.normal(size=shape).astype(np.float32) for _ in range(4))


def k8_bytes_per_sweep(n_sites):
    """What k8_sweep moves per sweep: two half-sweep launches, each reading the four disorder arrays whole (16 B per site: a
    line holds both colours; J_down[r-1] and J_layer[z-1] are other lanes' own rows and come from L2) and the spin rows (1 B per
    site, the four neighbour rows from L2) and writing them (1 B per site)."""
    return 2 * n_sites * (16 + 2)


def k7_bytes_per_sweep(n_sites):
    return 2 * n_sites * (12 + 2)


def timed(ctx, call, per_call, reps=5):
    """Median ms per sweep of `call(n_sweeps, sweep0)` (asynchronous), events around each call."""
    call(2, 0)
    ctx.synchronize()
    out, sw = [], 2
    for _ in range(reps):
        ctx.timer_begin()
        call(per_call, sw)
        out.append(ctx.timer_end() / per_call)
        sw += per_call
    return float(np.median(out))


def time_k8(L, per_call):
    ctx = _hip.Context.default()
    lat = _hip.Lattice3D(L, L, L, True, ctx=ctx)
    try:
        lat.randomize(3)
        lat.set_disorder(*disorder((L, L, L)))
        return timed(ctx, lambda n, sw: lat.sweep(T, n, 7, sw), per_call)
    finally:
        lat.close()


SHAPES = (((256, 256, 256), True), ((64, 256, 1024), True), ((16, 1024, 1024), True), ((1024, 1024, 16), True),
          ((1, 4096, 4096), (False, True, True)))


def time_shapes(out):
    """2^24 sites in other shapes: does the row width matter, and what do the loads of the layers z -+ 1 cost?"""
    ctx = _hip.Context.default()
    lines = []
    for shape, periodic in SHAPES:
        lat = _hip.Lattice3D(*shape, periodic, ctx=ctx)
        try:
            lat.randomize(3)
            d = disorder(shape)
            if periodic is not True:
                d[2][-1] = 0.0  # open z axis: no bond above the last layer
            lat.set_disorder(*d)
            ms = timed(ctx, lambda n, sw: lat.sweep(T, n, 7, sw), 16)
        finally:
            lat.close()
        N = int(np.prod(shape))
        lines.append(f"K8 {shape} periodic={periodic} 16 sweeps/call: {ms * 1e3:9.1f} us/sweep  {N / (ms * 1e-3):.3e} updates/s  "
                     f"{k8_bytes_per_sweep(N) / (ms * 1e-3) / 1e12:.2f} TB/s on 36 B per site and sweep")
        print(lines[-1], flush=True)
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "lattice3d_shapes.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def time_k7(L, per_call):
    ctx = _hip.Context.default()
    lat = _hip.Lattice(L, L, True, ctx=ctx)
    try:
        lat.randomize(3)
        lat.set_disorder(*disorder((L, L))[:3])
        return timed(ctx, lambda n, sw: lat.disorder_sweep(T, n, 7, sw), per_call)
    finally:
        lat.close()


def time_k5(L, reps=3, n=10):
    """K5 on the same Gaussian couplings: CSR of the 6-neighbour periodic lattice (built row by row: every site has exactly six
    neighbours), colour 0 then colour 1 (the checkerboard colouring)."""
    shape = (L, L, L)
    N = L ** 3
    jr, jd, jl, h = disorder(shape)
    idx = np.arange(N, dtype=np.int32).reshape(shape)
    nb, val = [], []
    for axis, J in ((2, jr), (1, jd), (0, jl)):
        nb.append(np.roll(idx, -1, axis=axis).ravel())   # bond J[i] to the next site of the axis
        val.append(J.ravel())
        nb.append(np.roll(idx, 1, axis=axis).ravel())    # bond J[i-1] to the previous one
        val.append(np.roll(J, 1, axis=axis).ravel())
    nb, val = np.stack(nb, axis=1), np.stack(val, axis=1).astype(np.float64)
    o = np.argsort(nb, axis=1, kind="stable")
    nb, val = np.take_along_axis(nb, o, axis=1), np.take_along_axis(val, o, axis=1)
    indptr = np.arange(N + 1, dtype=np.int64) * 6
    bias = 2.0 * h.ravel().astype(np.float64) - 2.0 * val.sum(axis=1)
    z, r, c = np.indices(shape)
    col = ((z + r + c) & 1).ravel()
    order = np.concatenate([np.flatnonzero(col == 0), np.flatnonzero(col == 1)]).astype(np.int32)
    offs = np.array([0, int((col == 0).sum()), N], np.int32)
    ctx = _hip.Context.default()
    g = _hip.SparseSystem(indptr, np.ascontiguousarray(nb.ravel()), 4.0 * val.ravel(), bias, offs, order, ctx=ctx)
    try:
        g.set_state(np.random.default_rng(1).integers(0, 2, size=N).astype(np.int8))
        g.sweep(T, 2, seed=3, sweep0=0)
        ctx.synchronize()
        best = []
        for rep in range(reps):
            ctx.timer_begin()
            g.sweep(T, n, seed=3, sweep0=2 + rep * n)
            best.append(ctx.timer_end() / n)
        return float(np.median(best)), 6 * N
    finally:
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--sizes", default="64,128,256")
    ap.add_argument("--no-k5", action="store_true")
    ap.add_argument("--no-k7", action="store_true")
    ap.add_argument("--shapes", action="store_true")
    a = ap.parse_args()
    if a.shapes:
        time_shapes(a.out)
        return
    rows, lines = [], []
    k8_at = {}
    for L in [int(x) for x in a.sizes.split(",")]:
        for per_call in (1, 16, 100):
            ms = time_k8(L, per_call)
            N = L ** 3
            ups, bw = N / (ms * 1e-3), k8_bytes_per_sweep(N) / (ms * 1e-3)
            k8_at[(L, per_call)] = ms
            rows.append(dict(route="k8", L=L, sweeps_per_call=per_call, ms_per_sweep=ms, updates_per_s=ups, bytes_per_s=bw,
                             hbm_fraction=bw / HBM_PEAK))
            lines.append(f"K8 {L}^3 gauss {per_call:3d} sweeps/call: {ms * 1e3:9.1f} us/sweep  {ups:.3e} updates/s  "
                         f"{bw / 1e12:.2f} TB/s (36 B per site and sweep) = {bw / HBM_PEAK:.2f} of HBM peak")
            print(lines[-1], flush=True)
    ref = k8_at.get((256, 16))
    if not a.no_k7:
        L = 4096
        for per_call in (1, 16, 100):
            ms = time_k7(L, per_call)
            ups, bw = L * L / (ms * 1e-3), k7_bytes_per_sweep(L * L) / (ms * 1e-3)
            rows.append(dict(route="k7", L=L, sweeps_per_call=per_call, ms_per_sweep=ms, updates_per_s=ups, bytes_per_s=bw,
                             hbm_fraction=bw / HBM_PEAK))
            lines.append(f"K7 {L}^2 gauss {per_call:3d} sweeps/call: {ms * 1e3:9.1f} us/sweep  {ups:.3e} updates/s  "
                         f"{bw / 1e12:.2f} TB/s (28 B per site and sweep)")
            if per_call == 16 and ref:
                lines[-1] += f"  | K8 256^3 / K7 4096^2 time = {ref / ms:.2f} (byte counts predict {36 / 28:.2f})"
            print(lines[-1], flush=True)
    if not a.no_k5:
        L = 256
        ms, nnz = time_k5(L)
        ups = L ** 3 / (ms * 1e-3)
        rows.append(dict(route="k5_csr", L=L, sweeps_per_call=10, ms_per_sweep=ms, updates_per_s=ups, nnz=nnz))
        lines.append(f"K5 CSR {L}^3 gauss (same couplings, checkerboard colouring): {ms * 1e3:9.1f} us/sweep  {ups:.3e} updates/s")
        if ref:
            rows[-1]["k5_over_k8"] = ms / ref
            lines[-1] += f"  | K5 / K8 (16 sweeps/call) time = {ms / ref:.2f}"
        print(lines[-1], flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "lattice3d_time.json"), "w") as f:
        json.dump(dict(T=T, hbm_peak=HBM_PEAK, device=_hip.Context.default().device_info(), rows=rows), f, indent=1)
    with open(os.path.join(a.out, "lattice3d_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

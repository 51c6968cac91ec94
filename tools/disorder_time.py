"""K7 disordered heat-bath sweeps: ms per sweep at 1024^2, 4096^2 and 8192^2 (periodic) for Gaussian bonds + fields and ±J bonds
without a field, at 1, 16 and 100 sweeps per call (device events after warm-up), with the bytes a sweep of K7 moves and the
fraction of HBM peak they reach; and the K5 CSR gather route (the general-graph kernel) on the same 4096^2 Gaussian couplings,
the route a disordered lattice had before K7.

    python tools/disorder_time.py [--out DIR] [--sizes 1024,4096,8192] [--no-k5]

Writes DIR/disorder_time.txt and DIR/disorder_time.json (default DIR: profiles/)."""
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


def disorder(L, kind, seed=1):
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        return tuple(rng.normal(size=(L, L)).astype(np.float32) for _ in range(3))
    jr, jd = (np.where(rng.random((L, L)) < 0.5, 1.0, -1.0).astype(np.float32) for _ in range(2))
    return jr, jd, None


def k7_bytes_per_sweep(L):
    """What k7_sweep moves per sweep: two half-sweep launches, each reading the three disorder planes whole (12 B per site:
    a line holds both colours) and the spin rows (1 B per site, neighbour rows from L2) and writing them (1 B per site)."""
    return 2 * L * L * (12 + 2)


def time_k7(L, kind, per_call, reps=5):
    ctx = _hip.Context.default()
    lat = _hip.Lattice(L, L, True, ctx=ctx)
    try:
        lat.randomize(3)
        lat.set_disorder(*disorder(L, kind))
        lat.disorder_sweep(T, 2, 7, 0)
        ctx.synchronize()
        lat.set_timing(True)
        best, sw = [], 2
        for _ in range(reps):
            lat.disorder_sweep(T, per_call, 7, sw)
            sw += per_call
            best.append(lat.last_sweep_ms() / per_call)
        return float(np.median(best))
    finally:
        lat.close()


def time_k5(L, reps=3, n=10):
    """K5 on the same Gaussian couplings: CSR of the 4-neighbour lattice, colour 0 then colour 1 (the checkerboard colouring)."""
    import scipy.sparse as sp
    from tsu.graph import canonical_csr
    jr, jd, h = disorder(L, "gauss")
    idx = np.arange(L * L, dtype=np.int64).reshape(L, L)
    r = np.concatenate([idx.ravel(), idx.ravel()])
    c = np.concatenate([np.roll(idx, -1, axis=1).ravel(), np.roll(idx, -1, axis=0).ravel()])
    v = np.concatenate([jr.ravel(), jd.ravel()]).astype(np.float64)
    J = sp.coo_matrix((v, (r, c)), shape=(L * L, L * L))
    A = canonical_csr(J + J.T)
    bias = 2.0 * h.ravel().astype(np.float64) - 2.0 * np.asarray(A.sum(axis=1)).ravel()
    col = ((idx // L + idx % L) & 1).ravel()
    order = np.concatenate([np.flatnonzero(col == 0), np.flatnonzero(col == 1)]).astype(np.int32)
    offs = np.array([0, int((col == 0).sum()), L * L], np.int32)
    ctx = _hip.Context.default()
    g = _hip.SparseSystem(A.indptr.astype(np.int64), A.indices.astype(np.int32), 4.0 * A.data, bias, offs, order, ctx=ctx)
    try:
        g.set_state(np.random.default_rng(1).integers(0, 2, size=L * L).astype(np.int8))
        g.sweep(T, 2, seed=3, sweep0=0)
        ctx.synchronize()
        best = []
        for rep in range(reps):
            ctx.timer_begin()
            g.sweep(T, n, seed=3, sweep0=2 + rep * n)
            best.append(ctx.timer_end() / n)
        return float(np.median(best)), int(A.nnz)
    finally:
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--sizes", default="1024,4096,8192")
    ap.add_argument("--no-k5", action="store_true")
    a = ap.parse_args()
    rows, lines = [], []
    for L in [int(x) for x in a.sizes.split(",")]:
        for kind in ("gauss", "pmJ"):
            for per_call in (1, 16, 100):
                ms = time_k7(L, kind, per_call)
                ups = L * L / (ms * 1e-3)
                bw = k7_bytes_per_sweep(L) / (ms * 1e-3)
                rows.append(dict(route="k7", L=L, disorder=kind, sweeps_per_call=per_call, ms_per_sweep=ms, updates_per_s=ups,
                                 bytes_per_s=bw, hbm_fraction=bw / HBM_PEAK))
                lines.append(f"K7 {L}^2 {kind:5s} {per_call:3d} sweeps/call: {ms * 1e3:9.1f} us/sweep  {ups:.3e} updates/s  "
                             f"{bw / 1e12:.2f} TB/s = {bw / HBM_PEAK:.2f} of HBM peak")
                print(lines[-1], flush=True)
    if not a.no_k5:
        L = 4096
        ms, nnz = time_k5(L)
        ups = L * L / (ms * 1e-3)
        rows.append(dict(route="k5_csr", L=L, disorder="gauss", sweeps_per_call=10, ms_per_sweep=ms, updates_per_s=ups, nnz=nnz))
        lines.append(f"K5 CSR {L}^2 gauss (same couplings, checkerboard colouring): {ms * 1e3:9.1f} us/sweep  {ups:.3e} updates/s")
        print(lines[-1], flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "disorder_time.json"), "w") as f:
        json.dump(dict(T=T, hbm_peak=HBM_PEAK, device=_hip.Context.default().device_info(), rows=rows), f, indent=1)
    with open(os.path.join(a.out, "disorder_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""K5 walker batches against the walker-by-walker route they replace, same graph, same process, the two sides alternating.

  colour route: a random graph of 2^20 sites, mean degree 6, with 1, 8 and 32 walkers at distinct temperatures; the batch's sweeps
      against that many SparseSystem.sweep calls (one per walker and window, on a resident state: no state copies are charged);
      32 walkers also with 4, 8 and 16 walkers per thread (TSU_K5B_CHUNK)
  small route: a 3-regular graph of 1000 sites, 256 walkers (16 ladders of 16), rounds of 10 sweeps with swaps; against 256 handles
      swept one by one, their energies read back one by one, and the swap pass on the host

Times are device-event times of windows that end in a synchronise (the handle loop's window: a host clock, it ends in its own energy
reads); every shape is warmed up first; REPEATS windows per side, median and minimum quoted, the ratio is between medians.
usage: sparse_batch_time.py [out.txt] [log2 n of the colour case]"""
import os
import sys
import time

sys.path.insert(0, "tsu-emulator_amd"); sys.path.insert(0, ".")
import numpy as np
import scipy.sparse as sp
from tsu import _hip as hip
from tsu.graph import canonical_csr, color_graph

REPEATS = 5
out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/sparse_batch_time.txt"
log2n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
ctx = hip.Context.default()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def random_graph(n, mean_degree, seed):
    rng = np.random.default_rng(seed)
    m = n * mean_degree // 2
    i, j = rng.integers(0, n, size=m), rng.integers(0, n, size=m)
    keep = i != j
    M = sp.coo_matrix((rng.normal(size=int(keep.sum())), (i[keep], j[keep])), shape=(n, n)).tocsr()
    return canonical_csr(M + M.T)


def cubic_graph(n, seed):
    """A ring plus a random perfect matching: 3-regular (a matched pair that is already a ring bond is drawn again)."""
    rng = np.random.default_rng(seed)
    while True:
        perm = rng.permutation(n)
        a, b = perm[: n // 2], perm[n // 2:]
        d = np.abs(a - b)
        if not np.any((d == 1) | (d == n - 1)):
            break
    ring = np.arange(n)
    rows, cols = np.concatenate([ring, a]), np.concatenate([(ring + 1) % n, b])
    M = sp.coo_matrix((rng.choice([-1.0, 1.0], size=rows.size), (rows, cols)), shape=(n, n)).tocsr()
    A = canonical_csr(M + M.T)
    assert np.all(np.diff(A.indptr) == 3)
    return A


def device_window(fn):
    ctx.timer_begin()
    fn()
    return ctx.timer_end()  # ms; synchronises


def stats(ts):
    return float(np.median(ts)), float(np.min(ts))


say(f"device: {ctx.device_info()['name']}  ({ctx.device_info()['compute_units']} CUs)")

# ---------------------------------------------------------------- colour route
n = 1 << log2n
A = random_graph(n, 6, 1)
bias = np.random.default_rng(2).normal(size=n)
offsets, order = color_graph(A)
say(f"colour route: random graph, n = 2^{log2n}, nnz = {A.nnz} (mean degree {A.nnz / n:.2f}), {len(offsets) - 1} colour classes")
single = hip.SparseSystem(A.indptr, A.indices, A.data, bias, offsets, order, ctx=ctx)
single.set_state(np.random.default_rng(3).integers(0, 2, size=n).astype(np.int8))
os.environ["TSU_K5B_SMALL"] = "0"
for nw, chunk in ((1, None), (8, None), (32, None), (32, 4), (32, 8), (32, 16)):
    if chunk is None:
        os.environ.pop("TSU_K5B_CHUNK", None)
    else:
        os.environ["TSU_K5B_CHUNK"] = str(chunk)
    temps = np.linspace(0.8, 3.0, nw) if nw > 1 else np.array([1.7])
    k = max(16, 128 // nw)  # sweeps per window
    batch = hip.SparseBatch(single, nw, 1)
    batch.set_temperatures(temps)
    batch.init(7, 0)
    w = batch.plan()["walkers_per_thread"]
    sweep0 = [0]

    def run_batch():
        batch.run(1, k, False, False)

    def run_single():
        for g in range(nw):
            single.sweep(float(temps[g]), k, seed=7, sweep0=sweep0[0], replica=g)
        sweep0[0] += k

    run_batch(); run_single(); ctx.synchronize()
    tb, ts = [], []
    for _ in range(REPEATS):
        tb.append(device_window(run_batch))
        ts.append(device_window(run_single))
    (mb, bb), (ms, bs) = stats(tb), stats(ts)
    upd = float(n) * nw * k
    say(f"  {nw:3d} walkers, {w:2d} per thread{' (forced)' if chunk else ''}, {k} sweeps per window: batch {mb:9.3f} ms (min {bb:9.3f}) = "
        f"{upd / (mb * 1e-3):.3e} walker-updates/s | walker by walker {ms:9.3f} ms (min {bs:9.3f}) = {upd / (ms * 1e-3):.3e} | "
        f"ratio {ms / mb:.2f}x")
    # one energy pass and one best-state pass at this size, for the record
    if chunk is None:
        batch.energies(); ctx.synchronize()
        te = [device_window(lambda: batch.energies()) for _ in range(REPEATS)]
        say(f"      energies of {nw} walkers (two launches + read-back): {stats(te)[0]:.3f} ms")
    batch.close()
os.environ.pop("TSU_K5B_CHUNK", None)
os.environ.pop("TSU_K5B_SMALL", None)
single.close()

# ---------------------------------------------------------------- small route
n, R, nl, interval, rounds = 1000, 16, 16, 10, 20
nw = R * nl
A = cubic_graph(n, 4)
bias = np.zeros(n)
offsets, order = color_graph(A)
temps = np.geomspace(0.5, 3.0, R)
say(f"small route: 3-regular graph, n = {n}, {len(offsets) - 1} colour classes, {nw} walkers ({nl} ladders of {R}), rounds of {interval} sweeps with swaps, "
    f"{rounds} rounds per window")
graph = hip.SparseSystem(A.indptr, A.indices, A.data, bias, offsets, order, ctx=ctx)
handles = [hip.SparseSystem(A.indptr, A.indices, A.data, bias, offsets, order, ctx=ctx) for _ in range(nw)]
rng = np.random.default_rng(5)
for h in handles:
    h.set_state(rng.integers(0, 2, size=n).astype(np.int8))
slot_T = np.tile(temps, nl)
counter = [0]


def run_handles():
    """The parent's route: a handle per walker, its energy read on the host, the swap pass on the host (temperatures move)."""
    for _ in range(rounds):
        for g, h in enumerate(handles):
            h.sweep(float(slot_T[g]), interval, seed=7, sweep0=counter[0], replica=g)
        E = np.array([h.energy()[0] for h in handles]).reshape(nl, R)
        T = slot_T.reshape(nl, R)
        for k in range(nl):
            idx = np.argsort(T[k])
            for i in range(R - 1):
                a, b = idx[i], idx[i + 1]
                d = (1.0 / T[k, a] - 1.0 / T[k, b]) * (E[k, a] - E[k, b])
                if d >= 0 or rng.random() < np.exp(d):
                    T[k, a], T[k, b] = T[k, b], T[k, a]
                    idx[i], idx[i + 1] = b, a
        counter[0] += interval


for label, env in (("small route", None), ("colour route forced (TSU_K5B_SMALL=0)", "0")):
    if env is None:
        os.environ.pop("TSU_K5B_SMALL", None)
    else:
        os.environ["TSU_K5B_SMALL"] = env
    batch = hip.SparseBatch(graph, R, nl)
    batch.set_temperatures(temps)
    batch.init(7, 0)

    def run_batch():
        batch.run(rounds, interval, True, False)

    run_batch(); ctx.synchronize()
    if env is None:
        run_handles()
    tb, th = [], []
    for _ in range(REPEATS):
        tb.append(device_window(run_batch))
        if env is None:
            t0 = time.perf_counter()
            run_handles()
            ctx.synchronize()
            th.append((time.perf_counter() - t0) * 1e3)
    upd = float(n) * nw * interval * rounds
    mb, bb = stats(tb)
    if env is None:
        mh, bh = stats(th)
        parent = (mh, bh)
        say(f"  {label}: batch {mb:9.3f} ms (min {bb:9.3f}) = {upd / (mb * 1e-3):.3e} walker-updates/s | handle by handle {mh:9.3f} ms (min {bh:9.3f}) = "
            f"{upd / (mh * 1e-3):.3e} | ratio {mh / mb:.1f}x | launches per round {batch.launch_count() // (rounds * (REPEATS + 1))}")
    else:
        say(f"  {label}: batch {mb:9.3f} ms (min {bb:9.3f}) = {upd / (mb * 1e-3):.3e} walker-updates/s | ratio to handle by handle {parent[0] / mb:.1f}x | "
            f"launches per round {batch.launch_count() // (rounds * (REPEATS + 1))}")
    batch.close()
os.environ.pop("TSU_K5B_SMALL", None)
for h in handles:
    h.close()
graph.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")

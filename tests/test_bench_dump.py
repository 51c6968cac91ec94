"""bench.py --dump-outputs: the files hold the lattice the timed steps computed, and --steps is the number of timed steps.

CPU part: the dump's layout, its byte budget and its fixed row sample, and the refusal of --steps < 1 (no torch import).
GPU part (-m gpu): bench.py run end to end on a small and on the default lattice; the dumped spins and observables must equal
the oracle's checkerboard sweeps from the same start (every sweep bench ran: warmup + timed steps)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bench_env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}


def test_dump_outputs_keeps_every_row_when_they_fit(tmp_path):
    b = _bench_module()
    spins = np.where(np.random.default_rng(1).random((40, 24)) < 0.5, 1, -1).astype(np.int8)
    b.dump_outputs(str(tmp_path), spins, (123, -456))
    got = np.load(tmp_path / "spins.npy")
    assert got.dtype == np.float32 and got.shape == (40, 24)
    np.testing.assert_array_equal(got, spins.astype(np.float32))
    np.testing.assert_array_equal(np.load(tmp_path / "spins_rows.npy"), np.arange(40, dtype=np.float64))
    obs = np.load(tmp_path / "observables.npy")
    assert obs.dtype == np.float64 and obs.tolist() == [123.0, -456.0]


def test_dump_outputs_samples_the_same_rows_within_the_budget(tmp_path):
    b = _bench_module()
    spins = np.where(np.random.default_rng(2).random((300, 64)) < 0.5, 1, -1).astype(np.int8)
    budget = 4 * 64 * 50  # 50 rows of float32
    for d in ("a", "b"):
        os.makedirs(tmp_path / d)
        b.dump_outputs(str(tmp_path / d), spins, None, name="s", budget=budget)
    rows = np.load(tmp_path / "a" / "s_rows.npy")
    assert rows.shape == (50,) and (np.diff(rows) > 0).all() and rows[-1] < 300
    np.testing.assert_array_equal(rows, np.load(tmp_path / "b" / "s_rows.npy"))
    got = np.load(tmp_path / "a" / "s.npy")
    assert got.nbytes <= budget
    np.testing.assert_array_equal(got, spins[rows.astype(np.int64)].astype(np.float32))
    assert not (tmp_path / "a" / "observables.npy").exists()
    # the default budget keeps bench's default lattice (4096^2) within 64 MB of files
    k = b.DUMP_SPIN_BYTES // (4 * 4096)
    assert k < 4096 and 4 * 4096 * k + 8 * k + 16 < 64e6


def test_bench_refuses_fewer_than_one_timed_step(tmp_path):
    r = subprocess.run([sys.executable, BENCH, "--steps", "0", "--dump-outputs", str(tmp_path / "d")], env=_bench_env(),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr and not r.stdout.strip()
    assert not (tmp_path / "d").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("L", [128, 4096])
def test_dumped_lattice_is_what_the_timed_steps_computed(tmp_path, L):
    from oracle import oracle as ora
    sps, warmup, steps = 8, 1, 3
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--L", str(L), "--steps", str(steps), "--warmup", str(warmup),
                        "--ramp-steps", "0", "--sweeps-per-step", str(sps), "--no-cpu-baseline", "--no-extra",
                        "--dump-outputs", str(out)], env=_bench_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["steps"] == steps and rec["ms_per_step"] > 0
    assert rec["config"]["launches"] >= 1 and rec["config"]["sweeps_per_step"] == sps
    table = ora.ising2d_thresholds(1.0, 0.0, _bench_module().T_C, ora.MODE_PHYSICAL)
    want = ora.ising2d_sweep(ora.ising2d_randomize(L, L, 42), True, table, (warmup + steps) * sps, 42, 0)
    rows = np.load(out / "spins_rows.npy").astype(np.int64)
    assert (rows.size == L) == (L == 128)
    np.testing.assert_array_equal(np.load(out / "spins.npy"), want[rows].astype(np.float32))
    assert np.load(out / "observables.npy").tolist() == [float(v) for v in ora.ising2d_observables(want, True)]
    assert sum(f.stat().st_size for f in out.iterdir()) <= 64e6

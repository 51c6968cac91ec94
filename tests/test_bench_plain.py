"""bench.py's plain run and --full: a plain run makes the main line only; --full adds the CPU baselines and the side
measurements after the timed steps.

CPU part: which side measurements a set of arguments asks for (no torch import).
GPU part (-m gpu): a plain run prints the main line with none of them."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_side_measurements_run_only_with_full():
    b = _bench_module()

    def plan(argv, world):
        return b.side_plan(b.build_parser().parse_args(argv), world)

    for world in (1, 2, 8):
        assert plan([], world) == set()
        assert plan(["--no-cpu-baseline", "--no-extra"], world) == set()
        assert plan(["--strong"], world) == set()
    assert plan(["--full"], 1) == {"cpu", "extra"}
    assert plan(["--full", "--no-extra"], 1) == {"cpu"}
    assert plan(["--full", "--no-cpu-baseline"], 1) == {"extra"}
    assert plan(["--full", "--no-cpu-baseline", "--no-extra"], 1) == set()
    # N > 1: the strong-scaling line beside the weak one; no CPU baselines
    assert plan(["--full"], 2) == {"strong"}
    assert plan(["--full", "--no-extra"], 2) == set()
    assert plan(["--full", "--strong"], 2) == set()


@pytest.mark.gpu
def test_plain_run_prints_the_main_line_only():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--L", "256", "--steps", "2", "--warmup", "1"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["unit"] == "spin-updates/s" and rec["higher_is_better"] is True and rec["dtype"] == "int8"
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["value"] > 0 and rec["ms_per_step"] > 0
    assert not any(key == "extra" or key.startswith("cpu_") for key in rec), sorted(rec)

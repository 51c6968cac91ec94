"""The arithmetic of a K2 call (csrc/dense_plan.h: routes, the plans of k2_own / k2_pipe / k2_coop, the kept-field state machine) is
plain host C++: tests/host/dense_plan_check.cpp exercises it as a stand-alone program, once plain and -- on a machine without a GPU --
once under the address and undefined-behaviour sanitizers.  Nothing of it is loaded into this process."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tsu-emulator_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "host", "dense_plan_check.cpp")


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:
        return not os.path.exists("/dev/kfd")


def _compilers():
    """The ROCm clang++ first (it links its sanitizer runtime statically), then the system's C++ compiler."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [c for c in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")) if os.path.exists(c)]
    return found[:1] + [c for c in (shutil.which("c++"),) if c]


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    errors = []
    for cxx in _compilers():
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, *flags, SOURCE, "-o", exe],
                           capture_output=True, text=True)
        if r.returncode == 0:
            break
        errors.append(f"{cxx}: {r.stderr[-2000:]}")
    else:
        pytest.fail("no C++17 compiler built dense_plan_check.cpp:\n" + "\n".join(errors))
    env = {k: v for k, v in os.environ.items() if not k.startswith("TSU_K2_")}  # (the program reads and sets these switches itself)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "0 failed" and len(lines) > 60 and all(line.startswith("ok  ") for line in lines[:-1])
    return lines


def test_dense_plan_header_needs_no_hip():
    text = open(os.path.join(CSRC, "dense_plan.h")).read()
    includes = re.findall(r"#\s*include\s*[<\"]([^>\"]+)", text)
    assert includes and all(re.fullmatch(r"c[a-z]+", h) for h in includes), includes  # (the C library's headers only)
    assert "dense_plan.h" in open(os.path.join(CSRC, "build.sh")).read()


def test_dense_plan_cases(tmp_path):
    _build_and_run(tmp_path, "dense_plan_check", [])


@pytest.mark.skipif(not _no_gpu(), reason="sanitizers run on a machine WITHOUT a GPU")
def test_dense_plan_cases_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "dense_plan_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])

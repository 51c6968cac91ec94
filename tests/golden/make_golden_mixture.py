#!/usr/bin/env python3
"""Generate tests/golden/g13_mixture.npz from the UNMODIFIED reference (the Gaussian-mixture energies of K3's mixture kernels).

Run where the reference is checked out (TSU_REFERENCE, as for make_golden.py), from outside the repository:

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python <repo>/tests/golden/make_golden_mixture.py

Two energies of the reference: MultimodalDistribution.energy (tsu/demos.py:73-87; 10-D, three modes drawn under
np.random.seed(13)) and MultimodalSampler.energy_function (tsu/api.py:143-149; 2-D, constructed with unnormalised weights,
which the sampler normalises).  For each: its centres and weights as the object holds them, about 40 points (near each centre,
between centres, on the 1e-10 plateau, far away), the reference's energies there and its _numerical_gradient (tsu/core.py:82-98).
Only arrays are stored.
"""
import os
import sys

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
REF = os.environ.get("TSU_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

import numpy as np  # noqa: E402

import tsu  # noqa: E402  (the reference)
from tsu.api import MultimodalSampler  # noqa: E402
from tsu.core import ThermalSamplingUnit  # noqa: E402
from tsu.demos import MultimodalDistribution  # noqa: E402

assert os.path.realpath(tsu.__file__).startswith(os.path.realpath(REF)), tsu.__file__
OUT = os.path.dirname(os.path.abspath(__file__))


def points(centers, rng):
    K, d = centers.shape
    pts = [c + 0.3 * rng.standard_normal(d) for c in centers for _ in range(3)]                      # near each centre
    pts += [0.5 * (centers[i] + centers[j]) + 0.2 * rng.standard_normal(d) for i in range(K) for j in range(i + 1, K)]
    pts += [(centers[i] + centers[j]) / 2 for i in range(K) for j in range(i + 1, K)]                   # between centres
    pts += [0.5 * rng.standard_normal(d) for _ in range(8)]                                             # the demo's starts
    spread = 1.0 + np.max(np.abs(centers))
    pts += [centers.mean(0) + 4.0 * spread * rng.standard_normal(d) for _ in range(8)]                  # plateau / far
    pts += [centers.mean(0) + 30.0 * rng.standard_normal(d) for _ in range(4)]                         # far away
    while len(pts) < 40:
        pts.append(centers[len(pts) % K] + rng.standard_normal(d))
    return np.array(pts[:40])


def case(energy, centers, weights, seed):
    rng = np.random.default_rng(seed)
    X = points(centers, rng)
    tsu_ = ThermalSamplingUnit()
    E = np.array([float(energy(x.copy())) for x in X])
    G = np.array([tsu_._numerical_gradient(energy, x.copy()) for x in X])
    return X, E, G


def main():
    np.random.seed(13)
    demo = MultimodalDistribution(dim=10)
    dc, dw = np.asarray(demo.mode_centers, float), np.asarray(demo.mode_weights, float)
    dX, dE, dG = case(demo.energy, dc, dw, 1)
    api = MultimodalSampler(centers=[[0.0, 0.0], [3.0, 3.0], [-2.0, 4.0]], weights=[1.0, 2.0, 3.0])
    ac, aw = np.array(api.centers, float), np.asarray(api.weights, float)
    aX, aE, aG = case(api.energy_function, ac, aw, 2)
    path = os.path.join(OUT, "g13_mixture.npz")
    np.savez_compressed(path, demo_centers=dc, demo_weights=dw, demo_x=dX, demo_energy=dE, demo_grad=dG,
                        api_centers=ac, api_weights=aw, api_weights_given=np.array([1.0, 2.0, 3.0]), api_x=aX, api_energy=aE,
                        api_grad=aG, demo_energy_at_zero=np.array(float(demo.energy(np.zeros(10)))))
    print("wrote", path, os.path.getsize(path), "bytes; E_demo(0) =", float(demo.energy(np.zeros(10))))


if __name__ == "__main__":
    main()

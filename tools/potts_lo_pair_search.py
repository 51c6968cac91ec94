#!/usr/bin/env python3
"""Find half-sweeps in which one octet of a Potts lattice holds two sites that the low half of u decides (no GPU needed).

K10's heat bath decides a site from hi16 of its uniform where it can and draws the octet's lo16 Philox block for the first site that
needs it; a second such site of the same octet reuses the block (`d.have_lo` in potts_site, csrc/potts_kern_dev.h).  That happens about
3e-7 times per octet and half-sweep, so no test meets it by chance.  With J = 0 the cumulative sums do not depend on the neighbours,
so the sites are known from Philox alone: this script walks the half-sweeps of a (rows, cols) lattice with the twin's own uniforms,
`cumulative` and `pick` (tests/helpers/potts_twin.py) and prints every (hs, global row, octet) that holds at least two of them.
The same rows and octets hold on a 3-D lattice with depth x rows = `--rows` global rows, whatever its colouring: u of octet
position m = (c >> 1) & 7 serves the site of either column parity.

tests/test_potts_far_end_cpu.py and tests/test_potts_far_end_gpu.py pin the first two finds of the default arguments:
hs = 2523 at (rho 104, octet 6) and hs = 9831 at (rho 114, octet 4).  About half a minute on one core.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELD8 = (0.5, -0.5, 0.25, 0.0, -0.25, 0.1, -0.1, 0.3)  # FIELDS[8] of the Potts tests


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=128, help="global rows (2-D: rows; 3-D: depth x rows)")
    ap.add_argument("--cols", type=int, default=128)
    ap.add_argument("--q", type=int, default=8)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--seed", type=lambda v: int(v, 0), default=0xFEDCBA9876543210)
    ap.add_argument("--replica", type=lambda v: int(v, 0), default=2 ** 24 - 1)
    ap.add_argument("--hs0", type=int, default=0, help="first half-sweep")
    ap.add_argument("--count", type=int, default=10000, help="half-sweeps to walk")
    ap.add_argument("--field", type=float, nargs="*", default=None, help="h_0 .. h_{q-1} (default: the tests' field at q = 8, else 0)")
    a = ap.parse_args()
    pt = _load("potts_twin")
    h = a.field if a.field else (FIELD8 if a.q == 8 else None)
    E, F = pt.tables(a.q, 0.0, h, a.temperature)
    none = np.zeros((a.rows, a.cols), np.int64)  # J = 0: E[n] = 1 for every n, so any neighbour count gives the same sums
    Z = pt.cumulative(E, F, [none] * a.q)
    found = 0
    for hs in range(a.hs0, a.hs0 + a.count):
        u = pt.site_uniforms(a.rows, a.cols, hs & 0xFFFFFFFF, a.seed, a.replica)
        mask = pt.lo_mask(Z, u)
        mask[:, 1::2] = False  # position m of an octet has one u, whichever column parity the half-sweep updates: count it once
        per_octet = pt.lo_octets(mask)
        for rho, o in np.argwhere(per_octet >= 2).tolist():
            cols = [c for c in range(16 * o, min(16 * o + 16, a.cols), 2) if pt.lo_mask([z[rho, c:c + 1] for z in Z], u[rho, c:c + 1])[0]]
            print(f"hs = {hs} (sweep {hs >> 1}, colour {hs & 1}): rho = {rho}, octet {o}, positions m = {[(c >> 1) & 7 for c in cols]}")
            found += 1
    print(f"{found} octets with two low-half sites in {a.count} half-sweeps of {a.rows} x {a.cols}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

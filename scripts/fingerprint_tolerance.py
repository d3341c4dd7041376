#!/usr/bin/env python
"""The measurement behind structure.FP_TOL, on the CPU from the float64 restatement tests/fp_ref64.py: on the crystals of the
golden fixtures g7 / g8 / g11, the fingerprint distance d between a crystal and copies rattled by Gaussian displacements of 0.02, 0.05 and
0.1 A, against d between distinct crystals of one formula (the same cell and composition with independently drawn coordinates; rock salt
against the CsCl type).  Usage: python scripts/fingerprint_tolerance.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from matinvent_amd.structure import lattice_matrix  # noqa: E402
from tests import fp_ref64 as R  # noqa: E402


def crystals():
    for name in ("g7_noise_loss", "g8_ft_step", "g11_noise_sampled_times"):
        z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        off = np.concatenate([[0], np.cumsum(z["num_atoms"])])
        for b in range(len(z["num_atoms"])):
            yield z["atom_types"][off[b]:off[b + 1]].astype(int), z["frac_coords"][off[b]:off[b + 1]].astype(np.float64), lattice_matrix(z["lengths"][b], z["angles"][b])


def main():
    g = np.random.default_rng(0)
    rattle = {0.02: [], 0.05: [], 0.1: []}
    distinct = []
    for t, x, L in crystals():
        if R.verdict(t, x, L)[0] != R.OK:
            continue
        u = R.fingerprint(t, x, L)["u"]
        for s in rattle:
            for _ in range(4):
                rattle[s].append(R.distance(u, R.fingerprint(t, x + g.normal(0, s, x.shape) @ np.linalg.inv(L), L)["u"]))
        for _ in range(4):
            distinct.append(R.distance(u, R.fingerprint(t, g.random(x.shape), L)["u"]))
    distinct.append(R.distance(R.fingerprint(*R.rock_salt())["u"], R.fingerprint(*R.cscl_type())["u"]))
    q = lambda v: "min %.4g  median %.4g  max %.4g  (n = %d)" % (np.min(v), np.median(v), np.max(v), len(v))
    for s, v in rattle.items():
        print(f"rattled by {s} A: {q(v)}")
    print(f"distinct, one formula: {q(distinct)}")


if __name__ == "__main__":
    main()

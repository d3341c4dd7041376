#!/usr/bin/env python
"""ms per call of structure.fingerprints at 64 and 256 crystals x 20 atoms, on a 3 A cubic cell (many translations per pair) and a 6 A
cubic cell (few), beside the numpy restatement's time for the same batch (tests/fp_ref64.py, float64, on the CPU; timed on 4 crystals and
scaled).  Prints one line per case and writes profiles/fingerprint_timing.json.  A measurement to record, not a gate.
Usage: python scripts/fingerprint_timing.py [--out profiles/fingerprint_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from matinvent_amd import structure  # noqa: E402
from tests import fp_ref64 as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fingerprint_timing.json"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    g = np.random.default_rng(0)
    results = []
    for cell in (3.0, 6.0):
        for B in (64, 256):
            n = 20
            types = torch.tensor(g.choice([3, 8, 26], B * n), dtype=torch.int32, device="cuda")
            frac = torch.tensor(g.random((B * n, 3)), dtype=torch.float32, device="cuda")
            lat = (torch.eye(3, device="cuda") * cell)[None].repeat(B, 1, 1).contiguous()
            na = torch.full((B,), n)
            for _ in range(3):
                fp, info = structure.fingerprints(na, types, frac, lat)
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            times = []
            for _ in range(a.reps):
                ev[0].record()
                fp, info = structure.fingerprints(na, types, frac, lat)
                ev[1].record()
                torch.cuda.synchronize()
                times.append(ev[0].elapsed_time(ev[1]))
            assert bool((info[:, 1] == 0).all())
            t0 = time.perf_counter()
            for b in range(4):
                R.fingerprint(types[b * n:(b + 1) * n].cpu().numpy(), frac[b * n:(b + 1) * n].cpu().numpy().astype(np.float64), lat[b].cpu().numpy().astype(np.float64))
            ref_ms = (time.perf_counter() - t0) / 4 * B * 1e3
            row = dict(cell=cell, crystals=B, atoms=n, images=float(info[0, 3]), ms_median=float(np.median(times)), ms_min=float(np.min(times)),
                       ms_max=float(np.max(times)), reps=a.reps, numpy_ref_ms=ref_ms)
            results.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), results=results), f, indent=1)


if __name__ == "__main__":
    main()

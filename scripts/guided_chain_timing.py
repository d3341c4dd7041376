"""Cost of a guided reverse step on the benchmark network (H 512, L 6, F 128, T = 1000 schedule; one property, 8 frequencies): ms per
reverse step of a guided chain (gamma != 0: two network evaluations per stage and one combination launch), of the gamma = 0 chain (the
conditional evaluation alone) and of the plain chain of the same property-conditioned model (the null row), all three alternating in one
process -- plain, gamma = 0, guided, plain, ... -- so that the yardstick is the plain chain of that process.

    python scripts/guided_chain_timing.py [--steps 6] [--rounds 3] [--json OUT]

64 and 256 crystals x 20 atoms, on one and on four streams.  Each measurement is the host wall clock of `steps` reverse steps from the top
of the schedule (sample(t_start=T, t_stop=T - steps)) with the device drained on both sides, after a warm-up call per form; per
configuration the median over `rounds` rounds.  Prints one JSON line per configuration.  The script asserts nothing about the outcome."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.gpu_util import Box, make_module  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from matinvent_amd.guidance import Guidance
    T, Fp = 1000, 8
    torch.manual_seed(0)
    sn = torch.cat([torch.ones(1), torch.linspace(1.2, 0.4, T)])
    m = make_module(512, 6, 128, T, None, sigmas_norm=sn, latent_dim=2 * Fp, condition=dict(properties=["y"], num_freqs=Fp))
    with torch.no_grad():   # (small heads: the states stay finite over the steps measured)
        v = m.decoder.views()
        for k in ("coord_out.weight", "lattice_out.weight", "type_out.weight", "type_out.bias"):
            v[k].mul_(0.1)
    m.decoder.mark_dirty()
    forms = {"plain": None, "gamma0": Guidance({"y": 0.5}, 0.0), "guided": Guidance({"y": 0.5}, 2.0)}
    rows = []
    for B in (64, 256):
        for streams in (1, 4):
            box = Box([20] * B)

            def run(g):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.sample(box, step_lr=5e-6, seed=1, t_start=T, t_stop=T - a.steps, streams=streams, **({} if g is None else {"guidance": g}))
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3 / a.steps
            for g in forms.values():
                run(g)
            ms = {k: [] for k in forms}
            for _ in range(a.rounds):
                for k, g in forms.items():
                    ms[k].append(run(g))
            med = {k: statistics.median(x) for k, x in ms.items()}
            row = dict(crystals=B, atoms=20, streams=streams, steps=a.steps, rounds=a.rounds, ms_per_step={k: round(x, 3) for k, x in med.items()},
                       all_ms_per_step={k: [round(y, 3) for y in x] for k, x in ms.items()},
                       guided_over_plain=round(med["guided"] / med["plain"], 3), gamma0_over_plain=round(med["gamma0"] / med["plain"], 3))
            print(json.dumps(row), flush=True)
            rows.append(row)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

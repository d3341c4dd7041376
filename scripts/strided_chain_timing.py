"""Wall time of one recorded rollout on the benchmark network (H 512, L 6, F 128, T = 1000, 20 atoms per crystal) on the full chain and on
strided chains of S = T/4 and T/10 steps (DiffCSPModule.respaced), and the time per step of each: the kernels of a step are the
same, so ms per step should not depend on S.

    python scripts/strided_chain_timing.py [--crystals 64,256] [--steps 1000,250,100] [--repeats 2] [--json OUT]

Prints one JSON line per (batch size, S): rollout seconds (the chain enqueued by sampling.sample_rollout's model.sample call with the
records kept, timed with events around it after one untimed warm-up chain of the same S), ms per step and structures per second."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import diffcsp_oracle as O  # noqa: E402
from tests.gpu_util import Box, make_module  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crystals", default="64,256")
    ap.add_argument("--atoms", type=int, default=20)
    ap.add_argument("--steps", default="1000,250,100")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    H, L, F, T = 512, 6, 128, 1000
    hp = O.CSPNetHParams(hidden_dim=H, num_layers=L, num_freqs=F)
    m = make_module(H, L, F, T, O.init_params(hp, seed=3, head_scale=0.01))
    rows = []
    for B in [int(x) for x in a.crystals.split(",")]:
        box = Box([a.atoms] * B)
        for S in [int(x) for x in a.steps.split(",")]:
            v = m.respaced(S)
            v.sample(box, step_lr=5e-6, seed=1, record=True, t_stop=max(0, S - 3))   # warm-up: handles, tables, workers
            torch.cuda.synchronize()
            best = None
            for r in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = v.sample(box, step_lr=5e-6, seed=2 + r, record=True)
                e1.record()
                torch.cuda.synchronize()
                del out
                ms = e0.elapsed_time(e1)
                best = ms if best is None else min(best, ms)
            row = dict(crystals=B, atoms=a.atoms, chain_steps=S, of_steps=T, rollout_s=round(best / 1e3, 4), ms_per_step=round(best / S, 4),
                       structures_per_s=round(B / best * 1e3, 1))
            print(json.dumps(row), flush=True)
            rows.append(row)
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

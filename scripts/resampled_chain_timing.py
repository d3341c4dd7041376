"""ms per reverse step of a RESAMPLED conditioned chain against the plain conditioned chain of the same build, on the benchmark network
(H 512, L 6, F 128, T = 1000, 20 atoms per crystal) through its 250-step view: the resampling jumps (DiffCSPModule.sample's `resample`;
DESIGN 37) add reverse steps -- RePaint's published setting, 250 steps with r = 10, j = 10, is 2410 reverse steps and 216 jumps -- and one
small launch per jump, resample_jump_kernel, of the predictor_kernel class.

    python scripts/resampled_chain_timing.py [--crystals 64,256] [--streams 1,4] [--sample-steps 250] [--t-start 250] [--resample 10,10]
                                             [--repeats 1] [--json OUT]

The condition fixes every atom type, the coordinates of every second atom and the lattice of every second crystal.  Both chains start at
step index `--t-start` of the view and run to 0, timed with events around the call after one untimed warm-up call of the plain chain (the
handles, tables and workers are the same for both); the calls' device synchronisation and host copies at attach time lie inside the timed
region, as a caller pays them.  Prints one JSON line per (batch size, streams): reverse steps and jumps of the schedule, ms per reverse
step of both chains, their ratio, and the whole resampled chain in seconds."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from matinvent_amd import resampling  # noqa: E402
from matinvent_amd.conditioning import Condition  # noqa: E402
from oracle import diffcsp_oracle as O  # noqa: E402
from tests.gpu_util import Box, make_module  # noqa: E402


def _condition(B, atoms, seed=0):
    g = torch.Generator().manual_seed(seed)
    N = B * atoms
    return Condition([atoms] * B, atom_types=torch.randint(1, 101, (N,), generator=g), known_types=torch.ones(N, dtype=torch.bool),
                     frac_coords=torch.rand(N, 3, generator=g), known_coords=torch.arange(N) % 2 == 0,
                     lattices=5 * torch.eye(3).repeat(B, 1, 1) + 0.3 * torch.randn(B, 3, 3, generator=g), known_lattice=torch.arange(B) % 2 == 0)


def _time(fn, repeats):
    best = None
    for _ in range(repeats):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        del out
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crystals", default="64,256")
    ap.add_argument("--atoms", type=int, default=20)
    ap.add_argument("--streams", default="1,4")
    ap.add_argument("--sample-steps", type=int, default=250)
    ap.add_argument("--t-start", type=int, default=None)
    ap.add_argument("--resample", default="10,10")
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    H, L, F, T = 512, 6, 128, 1000
    hp = O.CSPNetHParams(hidden_dim=H, num_layers=L, num_freqs=F)
    v = make_module(H, L, F, T, O.init_params(hp, seed=3, head_scale=0.01)).respaced(a.sample_steps)
    r, j = (int(x) for x in a.resample.split(","))
    t_start = a.sample_steps if a.t_start is None else a.t_start
    levels = resampling.schedule(t_start, r, j)
    steps = sum(1 for p, q in zip(levels[:-1], levels[1:]) if q == p - 1)
    jumps = len(levels) - 1 - steps
    rows = []
    for B in [int(x) for x in a.crystals.split(",")]:
        box, cond = Box([a.atoms] * B), _condition(B, a.atoms)
        for streams in [int(x) for x in a.streams.split(",")]:
            kw = dict(step_lr=5e-6, seed=2, t_start=t_start, streams=streams, condition=cond)
            v.sample(box, **{**kw, "t_start": min(t_start, 10)})   # warm-up: handles, tables, workers
            plain = _time(lambda: v.sample(box, **kw), a.repeats)
            resampled = _time(lambda: v.sample(box, resample=(r, j), **kw), a.repeats)
            row = dict(crystals=B, atoms=a.atoms, streams=streams, sample_steps=a.sample_steps, t_start=t_start, r=r, j=j, reverse_steps=steps, jumps=jumps,
                       ms_per_step_conditioned=round(plain / t_start, 4), ms_per_step_resampled=round(resampled / steps, 4),
                       ratio_per_step=round((resampled / steps) / (plain / t_start), 4), resampled_chain_s=round(resampled / 1e3, 3),
                       conditioned_chain_s=round(plain / 1e3, 3))
            print(json.dumps(row), flush=True)
            rows.append(row)
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

"""Cost of one preference (Diffusion-DPO) micro-step on the benchmark network (H 512, L 6, F 128, T = 1000): mi_dpo_micro_step against
mi_ft_micro_step on the same set, the same handles and in the same process.  The fine-tune entry is the reference figure: the two share
everything but the loss stage (three launches against two), so they should agree to within those launches.

    python scripts/dpo_step_timing.py [--crystals 64] [--atoms 20] [--pairs 64] [--iters 20] [--json OUT]

Prints one JSON line: ms per micro-step of both entries (device noise, the prior's forward forked onto a second stream as ft_step and
dpo_step do), and their ratio."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import diffcsp_oracle as O  # noqa: E402
from tests.gpu_util import make_module  # noqa: E402


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    from matinvent_amd import finetune, preference, streams
    from matinvent_amd.data import CrystalBatchData, CrystalData
    ap = argparse.ArgumentParser()
    ap.add_argument("--crystals", type=int, default=64)
    ap.add_argument("--atoms", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    H, L, F, T = 512, 6, 128, 1000
    hp = O.CSPNetHParams(hidden_dim=H, num_layers=L, num_freqs=F)
    P = O.init_params(hp, seed=3, head_scale=0.1)
    g = torch.Generator().manual_seed(5)
    agent = make_module(H, L, F, T, {k: v + 0.002 * torch.randn(v.shape, generator=g) for k, v in P.items()})
    prior = make_module(H, L, F, T, P)
    prior.requires_grad_(False)
    B, n = a.crystals, a.atoms
    data = [CrystalData(torch.rand(n, 3, generator=g), torch.randint(1, 95, (n,), generator=g), 4 + 6 * torch.rand(1, 3, generator=g),
                        70 + 40 * torch.rand(1, 3, generator=g)) for _ in range(B)]
    rewards = np.random.default_rng(0).random(B)
    batch = CrystalBatchData(data)
    batch.reward = torch.from_numpy(rewards).float()
    batch = batch.to("cuda")
    agent.shard_offsets = prior.shard_offsets = (0, 0)
    pairs = preference.build_pairs(rewards, max_pairs=a.pairs, seed=0)
    agent._batch_for(batch.num_atoms.cpu()).set_pairs(pairs)
    aux = streams.concurrent_streams(2, "cuda")[1]
    grad, stats = torch.zeros_like(agent.decoder.theta), torch.zeros(3, device="cuda")
    step = [0]

    def ft():
        step[0] += 1
        finetune._fused_micro_step(agent, prior, batch, step[0] % T, None, 0.025, B, 10, grad, stats, aux_stream=aux)

    def dpo():
        step[0] += 1
        preference._dpo_micro_step(agent, prior, batch, step[0] % T, None, 100.0, len(pairs), 10, grad, stats, aux_stream=aux)

    ms_ft = timed(ft, a.iters)
    ms_dpo = timed(dpo, a.iters)
    ms_ft2 = timed(ft, a.iters)
    row = dict(crystals=B, atoms=n, pairs=len(pairs), iters=a.iters, ms_ft_micro_step=round(ms_ft, 3), ms_dpo_micro_step=round(ms_dpo, 3),
               ms_ft_micro_step_again=round(ms_ft2, 3), dpo_over_ft=round(ms_dpo / (0.5 * (ms_ft + ms_ft2)), 4),
               finite=bool(torch.isfinite(grad).all() and torch.isfinite(stats).all()))
    print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()

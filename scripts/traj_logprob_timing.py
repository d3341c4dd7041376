"""Cost of DiffCSPModule.forward_logprb + its backward on the pinned network (H 512, L 6, F 128, T = 1000), against one fine-tune micro-step
at the same batch (module surface, pipeline/mat_invent.py:152-164: add_noise, the agent's loss, the prior's forward, the KL term, backward).

    python scripts/traj_logprob_timing.py [--crystals 256,64] [--iters 10] [--json OUT]

Prints one line per batch size: ms per forward_logprb + backward, ms per micro-step, their ratio, and the device memory the two taped
batch handles of forward_logprb hold (free device memory before / after their first taped call).  Under
`rocprofv3 --kernel-trace --stats -- python scripts/traj_logprob_timing.py ...` the stats file gives the two new kernels' share
(traj_logprob_kernel, traj_seed_kernel)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import diffcsp_oracle as O  # noqa: E402
from tests.gpu_util import Box, make_module  # noqa: E402


class FtBatch:
    def __init__(self, na, gen):
        B, N = len(na), sum(na)
        self.num_atoms = torch.tensor(na)
        self.num_graphs = B
        self.lengths, self.angles = 4 + 6 * torch.rand(B, 3, generator=gen), 70 + 40 * torch.rand(B, 3, generator=gen)
        self.frac_coords, self.atom_types = torch.rand(N, 3, generator=gen), torch.randint(1, 95, (N,), generator=gen)
        self.batch = torch.repeat_interleave(torch.arange(B), self.num_atoms).cuda()
        self.reward = torch.rand(B, generator=gen).cuda()


def timed(fn, iters):
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
    ap = argparse.ArgumentParser()
    ap.add_argument("--crystals", default="256,64")
    ap.add_argument("--atoms", type=int, default=20)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    H, L, F, T = 512, 6, 128, 1000
    hp = O.CSPNetHParams(hidden_dim=H, num_layers=L, num_freqs=F)
    P = O.init_params(hp, seed=3, head_scale=0.1)
    agent, prior = make_module(H, L, F, T, P), make_module(H, L, F, T, P)
    prior.requires_grad_(False)
    gen = torch.Generator().manual_seed(0)
    rows = []
    for B in [int(x) for x in a.crystals.split(",")]:
        na = [a.atoms] * B
        N = sum(na)
        t = T // 2
        init = (torch.rand(N, 3, generator=gen), 4 * torch.eye(3) + torch.randn(B, 3, 3, generator=gen), torch.randn(N, 100, generator=gen))
        _, traj = agent.sample(Box(na), step_lr=5e-6, seed=1, init=init, record=True, t_start=t, t_stop=t - 1)
        state = {k: traj[t][k].clone() for k in ("atom_types", "frac_coords", "frac_coords_mid", "lattices")}
        state.update(next_atom_types=traj[t - 1]["atom_types"].clone(), next_frac_coords=traj[t - 1]["frac_coords"].clone(),
                     next_lattices=traj[t - 1]["lattices"].clone(), num_atoms=torch.tensor(na), timesteps=torch.full((B,), t))
        w = torch.randn(3, B, generator=gen).cuda()
        torch.cuda.synchronize()
        free0, res0 = torch.cuda.mem_get_info()[0], torch.cuda.memory_reserved()

        def logprb():
            lp_l, lp_t, lp_x, _ = agent.forward_logprb(dict(state), step_lr=5e-6)
            ((w[0] * lp_l).sum() + (w[1] * lp_t).sum() + (w[2] * lp_x).sum()).backward()

        out = agent.forward_logprb(dict(state), step_lr=5e-6)   # first taped call: the handle pair and its tapes are allocated
        torch.cuda.synchronize()
        # the library's allocations (hipMalloc) = the drop in free memory not explained by torch's caching allocator
        handles_mb = (free0 - torch.cuda.mem_get_info()[0] - (torch.cuda.memory_reserved() - res0)) / 2 ** 20
        del out
        ms_lp = timed(logprb, a.iters)
        batch = FtBatch(na, gen)

        def micro_step():
            noised = agent.add_noise(batch, 500)
            sample_loss, agent_pred = agent.calc_sample_loss(noised)
            with torch.no_grad():
                _, prior_pred = prior.calc_sample_loss(noised)
            kl = agent.calc_kl_reg(agent_pred, prior_pred, batch)
            ((batch.reward * sample_loss + kl * (1.1 - batch.reward) * 0.025).mean()).backward()

        ms_ft = timed(micro_step, a.iters)
        row = dict(crystals=B, atoms=a.atoms, ms_forward_logprb_backward=round(ms_lp, 3), ms_ft_micro_step=round(ms_ft, 3),
                   ratio=round(ms_lp / ms_ft, 3), handles_mib=round(handles_mb, 1))
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

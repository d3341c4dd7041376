"""The fine-tune fixture shared by tests/test_gpu_optim_clip.py and the child processes it starts."""
import numpy as np, torch
from oracle import diffcsp_oracle as O
from tests.gpu_util import make_module
from matinvent_amd.data import CrystalData
from matinvent_amd.finetune import ft_step


def ft_fixture():
    """The 4-crystal fixture of tests/test_gpu_train.py::test_ft_step_end_to_end_vs_oracle: (make_agents, data, rewards, noise_fn, cfg)."""
    hp = O.CSPNetHParams(hidden_dim=64, num_layers=2, num_freqs=8)
    P0, Q0 = O.init_params(hp, seed=3), O.init_params(hp, seed=3)
    gen = torch.Generator().manual_seed(9)
    for k in P0:
        P0[k] = P0[k] + 0.01 * torch.randn(P0[k].shape, generator=gen)
    sn = torch.cat([torch.ones(1), 0.5 + torch.rand(1000, generator=gen)])

    def make_agents():
        agent, prior = make_module(64, 2, 8, 1000, P0, sigmas_norm=sn), make_module(64, 2, 8, 1000, Q0, sigmas_norm=sn)
        prior.requires_grad_(False)
        return agent, prior

    na = [4, 2, 6, 3]
    data = [CrystalData(torch.rand(n, 3, generator=gen), torch.randint(1, 95, (n,), generator=gen), 4 + 6 * torch.rand(1, 3, generator=gen),
                        70 + 40 * torch.rand(1, 3, generator=gen)) for n in na]
    rewards = torch.rand(len(na), generator=gen).numpy()
    B, N = len(na), sum(na)
    noises = {(e, t): (torch.randn(B, 3, 3, generator=gen), torch.randn(N, 3, generator=gen), torch.randn(N, 100, generator=gen))
              for e in range(2) for t in range(6)}
    cfg = dict(lr=1e-4, accum_steps=3, epochs=2, timesteps=6, sigma=0.025)
    return make_agents, data, rewards, (lambda e, t: noises[(e, t)]), cfg

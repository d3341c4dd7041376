"""Cost of one PPO-clipped policy-gradient micro-step on the benchmark network (H 512, L 6, F 128, T = 1000, 20 atoms per crystal): the fused
C entry (policy.pg_micro_step = mi_traj_pg_step: gather, two taped evaluations, surrogate and seeds, backward) against the unfused
composition on the same draws (torch indexing of the rollout, forward_logprb, the surrogate in torch, autograd).

    python scripts/pg_step_timing.py [--crystals 64,256] [--iters 10] [--logratio] [--sample-steps S] [--conditioned] [--json OUT]

Prints one JSON line per batch size: ms per micro-step and crystal-timesteps/s for both paths, next to DESIGN 21's forward_logprb + backward
(9.2 ms at 64 crystals, 20.7 ms at 256).  --logratio also re-evaluates EVERY step t = 2..T of the rollout at unchanged weights and reports the
largest |log rho| (the sampler's recorded log-probabilities against the re-evaluation: pure rounding), per term and for w = (1, 1, 1).
--sample-steps S runs all of it on the strided chain of S of the T steps (DiffCSPModule.respaced): rollout, draws and re-evaluation.
--conditioned also times the same micro-step on a handle pair that carries a likelihood mask (every atom type known, every
second atom's coordinates, every second crystal's lattice) and prints ms_masked beside ms_fused of the same build -- the masked kernels
do the unmasked kernels' work less the skipped terms, on the same rollout (its record is not the masked one: this is a timing, not a ratio).
Under `rocprofv3 --kernel-trace --stats -- python scripts/pg_step_timing.py ...` the stats file gives the gather and surrogate kernels' share
(traj_pg_gather_kernel, traj_pg_surrogate_kernel)."""
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

DESIGN21_MS = {64: 9.2, 256: 20.7}


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def rollout_of(m, na, seed):
    from matinvent_amd import sampling

    class Fixed:
        def __init__(self, total_num, dataset="mp_20"):
            self.num_atoms = np.asarray(na)

    orig = sampling.SampleDataset
    sampling.SampleDataset = Fixed
    try:
        return sampling.sample_rollout(len(na), m, seed=seed, geometric_filter=False)[1]
    finally:
        sampling.SampleDataset = orig


def main():
    from matinvent_amd import policy
    ap = argparse.ArgumentParser()
    ap.add_argument("--crystals", default="64,256")
    ap.add_argument("--atoms", type=int, default=20)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--logratio", action="store_true")
    ap.add_argument("--sample-steps", type=int, default=None, help="run on the strided chain of this many of the T = 1000 steps")
    ap.add_argument("--conditioned", action="store_true", help="also time the micro-step under a likelihood mask")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    H, L, F, T = 512, 6, 128, 1000
    hp = O.CSPNetHParams(hidden_dim=H, num_layers=L, num_freqs=F)
    m = make_module(H, L, F, T, O.init_params(hp, seed=3, head_scale=0.1))
    if a.sample_steps is not None:   # everything below through the view: T is its number of steps, every time a step index
        m = m.respaced(a.sample_steps)
        T = m.beta_scheduler.timesteps
    eps, w = 1e-4, np.ones(3, np.float32)
    rows = []
    for B in [int(x) for x in a.crystals.split(",")]:
        na = [a.atoms] * B
        ro = rollout_of(m, na, seed=1)
        torch.cuda.synchronize()
        rng = np.random.default_rng(0)
        draws = [rng.integers(2, T + 1, size=B).astype(np.int32) for _ in range(a.iters + 1)]
        draws_dev = [torch.from_numpy(d).cuda() for d in draws]
        A = torch.from_numpy(policy.advantages(rng.random(B))).cuda()
        M = B
        handles = (m.make_batch(na), m.make_batch(na))
        grad = torch.zeros_like(m.decoder.theta)
        stats = torch.zeros(4, B, device="cuda")

        def fused(i=0):
            policy.pg_micro_step(m, handles, ro, draws[i], draws_dev[i], A, eps, w, 1.0 / M, grad, stats)

        ms_fused = timed(fused, a.iters)
        ms_masked = None
        if a.conditioned:
            from matinvent_amd.conditioning import Condition
            N = sum(na)
            cond = Condition(na, atom_types=torch.ones(N, dtype=torch.long), known_types=torch.ones(N, dtype=torch.bool),
                             frac_coords=torch.zeros(N, 3), known_coords=torch.arange(N) % 2 == 0, lattices=torch.zeros(B, 3, 3),
                             known_lattice=torch.arange(B) % 2 == 0)
            masked = (m.make_batch(na), m.make_batch(na))
            for h in masked:
                cond.attach_likelihood(m, h)

            def fused_masked(i=0):
                policy.pg_micro_step(m, masked, ro, draws[i], draws_dev[i], A, eps, w, 1.0 / M, grad, stats)

            ms_masked = timed(fused_masked, a.iters)
            ms_fused = min(ms_fused, timed(fused, a.iters))   # (the unmasked step once more, after the masked one: same build, same box, interleaved)
            del masked
        ar_n, ar_b = torch.arange(sum(na), device="cuda"), torch.arange(B, device="cuda")
        nat = ro.num_atoms.cuda()

        def unfused(i=0):
            t = draws_dev[i].long()
            tn = torch.repeat_interleave(t, nat)
            st = dict(atom_types=ro.atom_types[tn, ar_n], frac_coords=ro.frac_coords[tn, ar_n], frac_coords_mid=ro.frac_coords_mid[tn, ar_n],
                      lattices=ro.lattices[t, ar_b].view(B, 3, 3), next_atom_types=ro.atom_types[tn - 1, ar_n],
                      next_frac_coords=ro.frac_coords[tn - 1, ar_n], next_lattices=ro.lattices[t - 1, ar_b].view(B, 3, 3),
                      num_atoms=ro.num_atoms, timesteps=t)
            lp_l, lp_t, lp_x, _ = m.forward_logprb(st, step_lr=ro.step_lr)
            o = ro.lp_old[t, ar_b]
            rho = torch.exp((lp_l + lp_t + lp_x) - o.sum(-1))
            loss = torch.maximum(-A * rho, -A * torch.clamp(rho, 1 - eps, 1 + eps)).sum() / M
            loss.backward()

        ms_unfused = timed(unfused, a.iters)
        m.decoder.theta.grad = None
        row = dict(crystals=B, atoms=a.atoms, chain_steps=T, ms_fused=round(ms_fused, 3), ms_unfused=round(ms_unfused, 3),
                   fused_over_unfused=round(ms_fused / ms_unfused, 4), crystal_timesteps_per_s_fused=round(B / ms_fused * 1e3, 1),
                   crystal_timesteps_per_s_unfused=round(B / ms_unfused * 1e3, 1), design21_forward_logprb_backward_ms=DESIGN21_MS.get(B))
        if ms_masked is not None:
            row.update(ms_masked=round(ms_masked, 3), masked_over_unmasked=round(ms_masked / ms_fused, 4))
        if a.logratio:
            # every step of the chain at unchanged weights: the largest |lp_new - lp_old| per term and for w = 1
            lp = torch.empty(3, B, device="cuda")
            worst = torch.zeros(4, device="cuda")
            for t in range(2, T + 1):
                th = np.full(B, t, np.int32)
                policy.pg_micro_step(m, handles, ro, th, torch.from_numpy(th).cuda(), A, eps, w, 0.0, grad, stats, lp)
                d = lp.t() - ro.lp_old[t]
                worst = torch.maximum(worst, torch.cat([d.abs().amax(0), d.sum(-1).abs().amax().view(1)]))
            wl = worst.tolist()
            row.update(max_abs_log_ratio=dict(l=wl[0], t=wl[1], x=wl[2], w111=wl[3]))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del handles, ro
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

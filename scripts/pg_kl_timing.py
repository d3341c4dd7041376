"""Cost of the KL anchor of the policy-gradient micro-step on the benchmark network (H 512, L 6, F 128, T = 1000, 20 atoms per crystal):
policy.pg_micro_step (mi_traj_pg_step, KL off) against policy.pg_kl_micro_step (mi_traj_pg_kl_step) with the prior's two inference
evaluations serial and on an auxiliary stream, next to one untaped forward_logprb (mi_traj_logprob, keep_tape = 0: two inference evaluations
and the log-probability kernel) on the same batch -- the yardstick of what the prior's two evaluations should cost.

    python scripts/pg_kl_timing.py [--crystals 64,256] [--iters 10] [--json OUT]

Prints one JSON line per batch size: ms per micro-step and crystal-timesteps/s of each form."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from oracle import diffcsp_oracle as O  # noqa: E402
from pg_step_timing import rollout_of, timed  # noqa: E402
from tests.gpu_util import make_module  # noqa: E402


def main():
    from matinvent_amd import policy
    from matinvent_amd.streams import concurrent_streams
    ap = argparse.ArgumentParser()
    ap.add_argument("--crystals", default="64,256")
    ap.add_argument("--atoms", type=int, default=20)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    H, L, F, T = 512, 6, 128, 1000
    hp = O.CSPNetHParams(hidden_dim=H, num_layers=L, num_freqs=F)
    P = O.init_params(hp, seed=3, head_scale=0.1)
    m = make_module(H, L, F, T, P)
    g = torch.Generator().manual_seed(4)
    prior = make_module(H, L, F, T, {k: v + 0.05 * (float(v.std()) if v.numel() > 1 else 0.0) * torch.randn(v.shape, generator=g)
                                     for k, v in P.items()})
    aux = concurrent_streams(2)[1]
    if aux == torch.cuda.current_stream():
        aux = concurrent_streams(2)[0]
    eps, w, beta = 0.2, np.ones(3, np.float32), 0.01
    rows = []
    for B in [int(x) for x in a.crystals.split(",")]:
        na = [a.atoms] * B
        ro = rollout_of(m, na, seed=1)
        torch.cuda.synchronize()
        rng = np.random.default_rng(0)
        draws = [rng.integers(2, T + 1, size=B).astype(np.int32) for _ in range(a.iters + 1)]
        draws_dev = [torch.from_numpy(d).cuda() for d in draws]
        A = torch.from_numpy(policy.advantages(rng.random(B))).cuda()
        handles = (m.decoder.make_batch(na), m.decoder.make_batch(na))
        ph = prior.decoder.make_batch(na)
        grad = torch.zeros_like(m.decoder.theta)
        stats4, stats5 = torch.zeros(4, B, device="cuda"), torch.zeros(5, B, device="cuda")

        def off(i=0):
            policy.pg_micro_step(m, handles, ro, draws[i], draws_dev[i], A, eps, w, 1.0 / B, grad, stats4)

        def serial(i=0):
            policy.pg_kl_micro_step(m, handles, prior, ph, ro, draws[i], draws_dev[i], A, eps, w, beta, 1.0 / B, grad, stats5)

        def on_aux(i=0):
            policy.pg_kl_micro_step(m, handles, prior, ph, ro, draws[i], draws_dev[i], A, eps, w, beta, 1.0 / B, grad, stats5, aux_stream=aux)

        # the yardstick: one untaped forward_logprb on a gathered batch of the same shape
        t = draws_dev[0].long()
        tn = torch.repeat_interleave(t, ro.num_atoms.cuda())
        an, ab = torch.arange(sum(na), device="cuda"), torch.arange(B, device="cuda")
        st = dict(atom_types=ro.atom_types[tn, an], frac_coords=ro.frac_coords[tn, an], frac_coords_mid=ro.frac_coords_mid[tn, an],
                  lattices=ro.lattices[t, ab].view(B, 3, 3), next_atom_types=ro.atom_types[tn - 1, an], next_frac_coords=ro.frac_coords[tn - 1, an],
                  next_lattices=ro.lattices[t - 1, ab].view(B, 3, 3), num_atoms=ro.num_atoms, timesteps=t)

        def untaped(i=0):
            with torch.no_grad():
                m.forward_logprb(st, step_lr=ro.step_lr)

        ms = {k: timed(f, a.iters) for k, f in (("kl_off", off), ("kl_serial", serial), ("kl_aux", on_aux), ("untaped_logprob", untaped))}
        row = dict(crystals=B, atoms=a.atoms, **{f"ms_{k}": round(v, 3) for k, v in ms.items()},
                   **{f"crystal_timesteps_per_s_{k}": round(B / v * 1e3, 1) for k, v in ms.items() if k != "untaped_logprob"},
                   added_ms_serial=round(ms["kl_serial"] - ms["kl_off"], 3), added_ms_aux=round(ms["kl_aux"] - ms["kl_off"], 3))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del handles, ph, ro
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

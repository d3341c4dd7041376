#!/usr/bin/env python
"""Generate g13_forward_logprb.npz by running the reference's own DiffCSPModule.sample and DiffCSPModule.forward_logprb.

Like make_golden.py (whose helpers it imports, and through it the reference modules via tests/oracle_shims), this runs only where the
reference checkout exists; the GPU tests read the committed npz alone.

g13: a small module (H 64, L 2, F 8, T = 20, heads scaled by 1e-2) samples three ragged crystals with torch's own generator -- on-distribution
states -- and forward_logprb re-evaluates the recorded steps t = T, T/2, 2 under the same weights.  Recorded per t: the state and the
next state it reads, the three log-probabilities, the corrector's predictions, and the fixed random weights w_* (on the log-probs) and v_*
(on the corrector's predictions) of the scalar sum(w_l lp_l + w_t lp_t + w_x lp_x) + sum(v_l pl) + sum(v_x px) + sum(v_t pt), whose
parameter gradient is accumulated over the three calls (one backward per call, as `.grad` accumulates) and recorded once; and the
predictor evaluation's outputs, which forward_logprb computes but does not return (the tests' error model needs the Normal means).
Usage: python tests/golden/make_golden_traj.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

STATE_KEYS = ("atom_types", "frac_coords", "frac_coords_mid", "lattices", "next_atom_types", "next_frac_coords", "next_lattices")


def g13_forward_logprb():
    T, step_lr = 20, 5e-6
    m = G.make_module(H=64, L=2, F=8, T=T, seed=13, head_scale=1e-2)
    num_atoms = [3, 5, 8]
    b = G.batch_of(num_atoms)
    B, N = b.num_graphs, b.num_nodes
    torch.manual_seed(1300)
    with torch.no_grad():
        _, traj = m.sample(b, step_lr=step_lr)
    g = torch.Generator().manual_seed(131)
    out = dict(num_atoms=b.num_atoms, T=np.array(T), step_lr=np.array(step_lr), time_freqs=G.time_freqs(256), ts=np.array([T, T // 2, 2]))
    m.zero_grad()
    for t in (T, T // 2, 2):
        state = dict(atom_types=traj[t]["atom_types"], frac_coords=traj[t]["frac_coords"], frac_coords_mid=traj[t]["frac_coords_mid"],
                     lattices=traj[t]["lattices"], num_atoms=b.num_atoms, timesteps=torch.full((B,), t, dtype=torch.long),
                     next_atom_types=traj[t - 1]["atom_types"], next_frac_coords=traj[t - 1]["frac_coords"],
                     next_lattices=traj[t - 1]["lattices"])
        state = {k: v.detach().clone() for k, v in state.items()}
        for k in STATE_KEYS:
            out[f"t{t}_{k}"] = state[k]
        w = {k: torch.randn(B, generator=g) for k in ("l", "t", "x")}
        v = dict(l=torch.randn(B, 3, 3, generator=g), x=torch.randn(N, 3, generator=g), t=torch.randn(N, 100, generator=g))
        lp_l, lp_t, lp_x, (pl, px, pt) = m.forward_logprb(dict(state), step_lr=step_lr)
        loss = (w["l"] * lp_l).sum() + (w["t"] * lp_t).sum() + (w["x"] * lp_x).sum() + (v["l"] * pl).sum() + (v["x"] * px).sum() + (v["t"] * pt).sum()
        loss.backward()
        out.update({f"t{t}_log_prob_l": lp_l, f"t{t}_log_prob_t": lp_t, f"t{t}_log_prob_x": lp_x,
                    f"t{t}_pred_l_corr": pl, f"t{t}_pred_x_corr": px, f"t{t}_pred_t_corr": pt})
        out.update({f"t{t}_w_{k}": a for k, a in w.items()})
        out.update({f"t{t}_v_{k}": a for k, a in v.items()})
        # the predictor evaluation's outputs forward_logprb computes inside (:197-204), for the tests' error model: a lattice / type-logit
        # mean of magnitude |m| is resolved to ulp(|m|) in fp32, which the Normal log-probabilities amplify by |x_next - m| / sigma^2
        with torch.no_grad():
            batch_idx = torch.repeat_interleave(torch.arange(B), b.num_atoms)
            pq = m.decoder(m.time_embedding(state["timesteps"]), state["atom_types"], state["frac_coords_mid"], state["lattices"], b.num_atoms,
                           batch_idx)
        out.update({f"t{t}_pred_l_pred": pq[0], f"t{t}_pred_x_pred": pq[1], f"t{t}_pred_t_pred": pq[2]})
        # the recorded log-probabilities of the chain at the same weights (forward_logprb reproduces them: a self-check of the fixture)
        for k in ("log_prob_l", "log_prob_t", "log_prob_x"):
            assert torch.allclose(out[f"t{t}_{k}"], traj[t][k], rtol=1e-4, atol=1e-4), (t, k)
    grads = {"G__decoder." + k: p.grad for k, p in m.decoder.named_parameters()}
    sd = {"P__" + k: a for k, a in m.state_dict().items()}
    G.npz("g13_forward_logprb", **out, **sd, **grads)


if __name__ == "__main__":
    g13_forward_logprb()

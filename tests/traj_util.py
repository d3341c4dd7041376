"""The oracle side of DiffCSPModule.forward_logprb (models/diffcsp/diffusion.py:158-227), written out on top of
oracle.diffcsp_oracle.cspnet_forward, for the trajectory log-probability tests (CPU and GPU).

Generalised in one respect, like the device path: crystal b is evaluated at its own timesteps[b] (scalars gathered per crystal);
with equal timesteps every quantity is the reference's, computed by the same fp32 operations."""
import torch

from oracle import diffcsp_oracle as O

STATE_KEYS = ("atom_types", "frac_coords", "frac_coords_mid", "lattices", "next_atom_types", "next_frac_coords", "next_lattices")


def time_embedding(times, freqs):
    e = times[:, None] * freqs[None, :]
    return torch.cat((e.sin(), e.cos()), dim=-1)


def forward_logprb(P, hp, beta, sigma, sigma_begin, state, step_lr, freqs=None):
    """beta: dict alphas / alphas_cumprod / sigmas; sigma: dict sigmas / sigmas_norm.  Returns (lp_l, lp_t, lp_x, (pl, px, pt))."""
    t = state["timesteps"].long()
    num_atoms = state["num_atoms"].long()
    B = len(num_atoms)
    batch = torch.repeat_interleave(torch.arange(B), num_atoms)
    time_emb = O.time_embedding(t, hp.time_dim) if freqs is None else time_embedding(t, freqs)
    at, x, xm, lat = state["atom_types"], state["frac_coords"], state["frac_coords_mid"], state["lattices"]
    alphas, alphas_cumprod = beta["alphas"][t], beta["alphas_cumprod"][t]
    c0 = 1.0 / torch.sqrt(alphas)
    c1 = (1 - alphas) / torch.sqrt(1 - alphas_cumprod)
    sigmas = beta["sigmas"][t]
    sigma_x, sigma_norm = sigma["sigmas"][t], sigma["sigmas_norm"][t]
    per_atom = lambda v: v[batch][:, None]   # a per-crystal scalar broadcast over an [N, k] tensor
    per_lat = lambda v: v[:, None, None]

    step_size = step_lr * (sigma_x / sigma_begin) ** 2                                       # :171
    std_x = torch.sqrt(2 * step_size)
    pl_c, px_c, pt_c = O.cspnet_forward(P, hp, time_emb, at, x, lat, num_atoms, batch)
    mu = (x - per_atom(step_size) * (px_c * per_atom(torch.sqrt(sigma_norm)))) % 1.0
    lp_xc = O.scatter_mean(O.log_prob_wn(xm, mu, per_atom(std_x)).mean(dim=-1), batch, B)

    adj = sigma["sigmas"][t - 1]                                                             # :194-196
    step_size = sigma_x ** 2 - adj ** 2
    std_x = torch.sqrt((adj ** 2 * (sigma_x ** 2 - adj ** 2)) / (sigma_x ** 2))
    pl_p, px_p, pt_p = O.cspnet_forward(P, hp, time_emb, at, xm, lat, num_atoms, batch)
    mu = (xm - per_atom(step_size) * (px_p * per_atom(torch.sqrt(sigma_norm)))) % 1.0
    lp_xp = O.scatter_mean(O.log_prob_wn(state["next_frac_coords"], mu, per_atom(std_x)).mean(dim=-1), batch, B)

    lp_l = O.normal_log_prob(state["next_lattices"], per_lat(c0) * (lat - per_lat(c1) * pl_p), per_lat(sigmas)).mean(dim=-1).mean(dim=-1)
    lp_t = O.scatter_mean(O.normal_log_prob(state["next_atom_types"], per_atom(c0) * (at - per_atom(c1) * pt_p), per_atom(sigmas)).mean(dim=-1),
                          batch, B)
    return lp_l, lp_t, lp_xc + lp_xp, (pl_c, px_c, pt_c)


def hparams_of(P):
    """CSPNetHParams of a `decoder.*` parameter dict (hidden width, layers, Fourier frequencies)."""
    H = P["decoder.node_embedding.weight"].shape[0]
    L = sum(1 for k in P if k.startswith("decoder.csp_layer_") and k.endswith("edge_mlp.0.weight"))
    F = (P["decoder.csp_layer_0.edge_mlp.0.weight"].shape[1] - 2 * H - 9) // 6
    return O.CSPNetHParams(hidden_dim=H, num_layers=L, num_freqs=F)

"""The per-step transition KL of the KL-anchored policy gradient (mi_traj_pg_kl_step) written out in float64 torch: the step
scalars of a recorded step per crystal, the closed form KL(p_agent(x_{t-1} | x_t) || p_prior(x_{t-1} | x_t)) from the two networks'
predictions, its local derivatives, and the float64 oracle of both networks' predictions on top of oracle.diffcsp_oracle.cspnet_forward.
Shared by the CPU and the GPU tests."""
import torch

from oracle import diffcsp_oracle as O
from tests.traj_util import time_embedding


def step_scalars(beta, sigma, sigma_begin, t, step_lr, dtype=torch.float64):
    """Crystal b's step scalars at t[b] (the quantities of tests/traj_util.forward_logprb), float64 [B] each.  dtype=torch.float32: the
    same expressions as separately rounded float32 tensor ops on the float32 tables, as the reference and sampler_coefficients form them."""
    t = torch.as_tensor(t).long()
    d = lambda v: v.to(dtype)
    alphas, alphas_cumprod = d(beta["alphas"][t]), d(beta["alphas_cumprod"][t])
    sx, sn, adj = d(sigma["sigmas"][t]), d(sigma["sigmas_norm"][t]), d(sigma["sigmas"][t - 1])
    step_corr = step_lr * (sx / sigma_begin) ** 2
    step_pred = sx ** 2 - adj ** 2
    return dict(c0=1.0 / torch.sqrt(alphas), c1=(1 - alphas) / torch.sqrt(1 - alphas_cumprod), sigma=d(beta["sigmas"][t]),
                sqrt_sn=torch.sqrt(sn), step_corr=step_corr, std_corr=torch.sqrt(2 * step_corr), step_pred=step_pred,
                std_pred=torch.sqrt(adj ** 2 * step_pred / sx ** 2))


def min_image(d):
    """d - rint(d): the nearest image of a difference of two points of the unit torus (torch.round rounds half to even, as rint)."""
    return d - torch.round(d)


def kl_terms(s, num_atoms, pl_a, pl_p, pt_a, pt_p, pxc_a, pxc_p, pxp_a, pxp_p):
    """(KL_l, KL_t, KL_x) [B] each.  s: step_scalars; pl [B,3,3], pt [N,A] (predictor heads), pxc / pxp [N,3] (the corrector's and the
    predictor's coordinate heads), _a the agent's, _p the prior's."""
    num_atoms = torch.as_tensor(num_atoms).long()
    B = len(num_atoms)
    batch = torch.repeat_interleave(torch.arange(B), num_atoms)
    cc = s["c0"] * s["c1"]
    var = s["sigma"] ** 2
    dl = cc[:, None, None] * (pl_a - pl_p)
    kl_l = (dl ** 2 / (2 * var[:, None, None])).mean(dim=(-1, -2))
    dt = cc[batch][:, None] * (pt_a - pt_p)
    kl_t = O.scatter_mean((dt ** 2 / (2 * var[batch][:, None])).mean(dim=-1), batch, B)
    kl_x = 0
    for step, std, a, p in (("step_corr", "std_corr", pxc_a, pxc_p), ("step_pred", "std_pred", pxp_a, pxp_p)):
        k = (s[step] * s["sqrt_sn"])[batch][:, None]
        d = min_image(k * (a - p))
        kl_x = kl_x + O.scatter_mean((d ** 2 / (2 * s[std][batch][:, None] ** 2)).mean(dim=-1), batch, B)
    return kl_l, kl_t, kl_x


def kl_derivatives(s, num_atoms, pl_a, pl_p, pt_a, pt_p, pxc_a, pxc_p, pxp_a, pxp_p):
    """The closed-form local derivatives d KL_k / d(agent prediction): (d pl_a, d pt_a, d pxc_a, d pxp_a)."""
    num_atoms = torch.as_tensor(num_atoms).long()
    B = len(num_atoms)
    batch = torch.repeat_interleave(torch.arange(B), num_atoms)
    n = num_atoms.clamp(min=1).double()[batch][:, None]
    cc2 = (s["c0"] * s["c1"]) ** 2
    var = s["sigma"] ** 2
    g_l = (cc2 / var)[:, None, None] * (pl_a - pl_p) / 9
    g_t = (cc2 / var)[batch][:, None] * (pt_a - pt_p) / (100 * n)
    out = [g_l, g_t]
    for step, std, a, p in (("step_corr", "std_corr", pxc_a, pxc_p), ("step_pred", "std_pred", pxp_a, pxp_p)):
        k = (s[step] * s["sqrt_sn"])[batch][:, None]
        out.append(min_image(k * (a - p)) * k / (3 * n * s[std][batch][:, None] ** 2))
    return tuple(out)


def predictions(P, hp, state, freqs):
    """Float64 oracle of one network on a recorded step: (pl, pt, pxp) of the predictor input and pxc of the corrector input."""
    t = state["timesteps"].long()
    num_atoms = state["num_atoms"].long()
    batch = torch.repeat_interleave(torch.arange(len(num_atoms)), num_atoms)
    P = {k: v.double() if not v.requires_grad else v for k, v in P.items()}
    temb = time_embedding(t.double(), freqs.double())
    at, lat = state["atom_types"].double(), state["lattices"].double()
    _, pxc, _ = O.cspnet_forward(P, hp, temb, at, state["frac_coords"].double(), lat, num_atoms, batch)
    pl, pxp, pt = O.cspnet_forward(P, hp, temb, at, state["frac_coords_mid"].double(), lat, num_atoms, batch)
    return pl, pt, pxc, pxp


def oracle_kl(Pa, Pp, hp, beta, sigma, sigma_begin, state, step_lr, freqs):
    """(KL_l, KL_t, KL_x) [B] of the agent's parameters Pa against the prior's Pp, float64, differentiable with respect to Pa."""
    s = step_scalars(beta, sigma, sigma_begin, state["timesteps"], step_lr)
    pl_a, pt_a, pxc_a, pxp_a = predictions(Pa, hp, state, freqs)
    with torch.no_grad():
        pl_p, pt_p, pxc_p, pxp_p = predictions(Pp, hp, state, freqs)
    return kl_terms(s, state["num_atoms"], pl_a, pl_p, pt_a, pt_p, pxc_a, pxc_p, pxp_a, pxp_p)

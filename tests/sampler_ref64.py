"""Float64 reference of the reverse sampler's own arithmetic (matinvent_amd/csrc/sampler.hip: corrector_kernel, predictor_kernel,
mi_sampler_init_state and the two wrap kernels) with no network and no device code in it: one reverse step at time t from given
predictions and given noise (diffusion.py:320-386 as sampler.hip restates it) and the initial state from the host Philox contract
(oracle.diffcsp_oracle.philox_*).  `step` takes the predictions as an argument, so a test that knows them exactly -- zero head weights:
pred_x = 0, pred_l = 0, pred_t = type_out.bias -- holds a yardstick without network error.  Called with dtype=float32 it is that
yardstick: the same formulas as separately rounded float32 tensor ops (the naive 21-image sum and torch's `% 1.`, as the reference).
The step scalars are kl_util.step_scalars, the wrapped normal, the Normal and the crystal mean are traj_ref64's.

Also here: the states and the noise those tests run on (build_step_state, build_noise), written so that the cell boundary is crossed where
a kernel can lose it, and oracle_step: oracle.diffcsp_oracle.sample restricted to one step on the same inputs in a chosen precision
(float64: what pins this file; float32: the yardstick of the non-zero-heads case).  Plain torch, CPU; shared by the CPU and the GPU tests."""
import os

import numpy as np
import torch

from oracle import diffcsp_oracle as O
from tests.kl_util import step_scalars
from tests.traj_ref64 import LAST_BELOW_ONE, NUM_TYPES, _batch, _crystal_mean, _normal, wrapped_normal  # noqa: F401

T = 1000
SIGMA_BEGIN, SIGMA_END = 0.005, 0.5
STEP_LR = 5e-6
HAIR = 1e-9                          # the hair-below-zero elements: x = 0, zero prediction, z = -HAIR / std
NOISE_KEYS = ("corr_x", "pred_x", "pred_l", "pred_t")
SIGMAS_NORM = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "matinvent_amd", "data",
                           "sigmas_norm_T1000_b0.005_e0.5_seed1234.npy")


def tables():
    """(beta, sigma) table dicts of the workload's T = 1000 schedule: cosine betas and the packaged sigmas_norm table."""
    sn = torch.from_numpy(np.load(SIGMAS_NORM)).float()
    assert sn.shape == (T + 1,)
    return O.beta_tables(T), O.sigma_tables(T, SIGMA_BEGIN, SIGMA_END, sigmas_norm=sn)


def scalars(tabs, t, B, dtype=torch.float64, step_lr=STEP_LR):
    """kl_util.step_scalars of B crystals all at time t."""
    return step_scalars(tabs[0], tabs[1], SIGMA_BEGIN, torch.full((B,), int(t)), step_lr, dtype)


def corrector(s, x, px_corr, z, num_atoms, keep_coords=False):
    """(drift, x_mid) of the corrector half (diffusion.py:320-334), both unwrapped: drift = x - step_corr sqrt(sn) px,
    x_mid = drift + std_corr z; CSP mode: x_mid = x.  z = None: no noise (t = 1)."""
    _, batch = _batch(num_atoms)
    pa = lambda k: s[k][batch][:, None]
    drift = x - pa("step_corr") * (px_corr * pa("sqrt_sn"))
    if keep_coords:
        return drift, x
    return drift, (drift if z is None else drift + pa("std_corr") * z)


def step(s, state, preds, z, keep_lattice=False, keep_coords=False, dtype=torch.float64):
    """One reverse step.  s: step scalars per crystal (any precision; taken to `dtype`); state: dict(frac_coords [N,3] in [0, 1),
    lattices [B,3,3], atom_types [N,100], num_atoms); preds = (px_corr [N,3], pl [B,3,3], px_pred [N,3], pt [N,100]): the corrector
    evaluation's coordinate head and the predictor evaluation's three heads; z = dict(corr_x, pred_x, pred_l, pred_t), or None at
    t = 1, where the reference draws no noise and records no log-probabilities.  Returns a dict:
      x_mid_raw, frac_raw    the corrector's and the predictor's coordinates before any wrap;
      x_mid = x_mid_raw % 1 (traj[t]['frac_coords_mid']),  frac_coords = ((frac_raw % 1) % 1) (the state and traj[t-1]);
      lattices, atom_types   the next state;     lp_l, lp_t, lp_x [B] (absent when z is None).
    float64: the wrapped normal through logsumexp (traj_ref64.wrapped_normal); float32: the reference's naive 21-image sum."""
    c = lambda v: v.to(dtype)
    s = {k: c(v) for k, v in s.items()}
    na, batch = _batch(state["num_atoms"])
    pa = lambda k: s[k][batch][:, None]
    pb = lambda k: s[k][:, None, None]
    px_c, pl, px_p, pt = (c(v) for v in preds)
    x, lat, at = c(state["frac_coords"]), c(state["lattices"]), c(state["atom_types"])
    zz = (lambda k: None) if z is None else (lambda k: c(z[k]))
    exact = dtype == torch.float64
    wn = (lambda v, mu, std: wrapped_normal(v, mu, std.expand_as(v))[0]) if exact else O.log_prob_wn
    normal = (lambda v, mu, sg: _normal(v, mu, sg.expand_as(v))[0]) if exact else O.normal_log_prob
    mean = lambda v: _crystal_mean(v.mean(dim=-1), batch, na)

    drift_c, xm = corrector(s, x, px_c, zz("corr_x"), na, keep_coords)
    drift_p = xm - pa("step_pred") * (px_p * pa("sqrt_sn"))
    raw = xm if keep_coords else (drift_p if z is None else drift_p + pa("std_pred") * zz("pred_x"))
    v = raw % 1.0
    mu_l, mu_t = pb("c0") * (lat - pb("c1") * pl), pa("c0") * (at - pa("c1") * pt)
    l_next = lat if keep_lattice else (mu_l if z is None else mu_l + pb("sigma") * zz("pred_l"))
    t_next = mu_t if z is None else mu_t + pa("sigma") * zz("pred_t")
    out = dict(x_mid_raw=xm, x_mid=xm % 1.0, frac_raw=raw, frac_coords=v % 1.0, lattices=l_next, atom_types=t_next)
    if z is not None:
        out["lp_l"] = normal(l_next, mu_l, pb("sigma")).mean(dim=-1).mean(dim=-1)
        out["lp_t"] = mean(normal(t_next, mu_t, pa("sigma")))
        out["lp_x"] = mean(wn(xm % 1.0, drift_c % 1.0, pa("std_corr"))) + mean(wn(v, drift_p % 1.0, pa("std_pred")))
    return out


def zero_head_preds(num_atoms, bias):
    """The predictions of a network whose three head weight matrices are zero, as step's preds (float64)."""
    na, _ = _batch(num_atoms)
    B, N = len(na), int(na.sum())
    zx = torch.zeros(N, 3, dtype=torch.float64)
    return zx, torch.zeros(B, 3, 3, dtype=torch.float64), zx, bias.double()[None, :].expand(N, NUM_TYPES)


def init_state(seed, T, num_atoms, node_offset=0, graph_offset=0):
    """(x_T [N,3] uniform, l_T [B,3,3] normal, t_T [N,100] normal) of the host Philox contract for a shard that starts at atom
    node_offset, crystal graph_offset: draws 0, 1, 2, step field T + 1, element ids node_offset*3 + i, graph_offset*9 + i,
    node_offset*100 + i."""
    na, _ = _batch(num_atoms)
    B, N = len(na), int(na.sum())
    f = lambda a, *shape: torch.from_numpy(np.ascontiguousarray(a)).view(*shape)
    return (f(O.philox_uniform(seed, T + 1, O.DRAW_X_T, N * 3, node_offset * 3), N, 3),
            f(O.philox_normal(seed, T + 1, O.DRAW_L_T, B * 9, graph_offset * 9), B, 3, 3),
            f(O.philox_normal(seed, T + 1, O.DRAW_T_T, N * NUM_TYPES, node_offset * NUM_TYPES), N, NUM_TYPES))


def philox_noise(seed, t, num_atoms, node_offset=0, graph_offset=0):
    """The host contract's four draws of step t for that shard, as step's z (float32)."""
    na, _ = _batch(num_atoms)
    B, N = len(na), int(na.sum())
    f = lambda draw, n, off, *shape: torch.from_numpy(np.ascontiguousarray(O.philox_normal(seed, t, draw, n, off))).view(*shape)
    return dict(corr_x=f(O.DRAW_CORR_X, N * 3, node_offset * 3, N, 3), pred_x=f(O.DRAW_PRED_X, N * 3, node_offset * 3, N, 3),
                pred_l=f(O.DRAW_PRED_L, B * 9, graph_offset * 9, B, 3, 3),
                pred_t=f(O.DRAW_PRED_T, N * NUM_TYPES, node_offset * NUM_TYPES, N, NUM_TYPES))


# ---- the states and the noise ---------------------------------------------------------------------------------------------------------

def boundary(num_atoms):
    """The flat [N*3] indices of the forced coordinates: (first, last, hair_corr, hair_pred).  first / last: every crystal's first and
    last coordinate (a one-atom crystal: x and z of its atom) -- the last one lies in the last, partial trip of the corrector's
    `idx += 64` and of the predictor's `idx += 256` loop.  hair_corr / hair_pred: the last coordinate but one of the largest and of the
    second largest crystal with at least two atoms (LOOP_NA: local index 511 of the 171-atom crystal, in the corrector's ninth trip,
    and local index 256 of the 86-atom crystal, in the predictor's second)."""
    na, _ = _batch(num_atoms)
    off = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(na, 0)])
    first, last = 3 * off[:-1], 3 * off[1:] - 1
    order = sorted((b for b in range(len(na)) if int(na[b]) >= 2), key=lambda b: (-int(na[b]), b))
    return first, last, int(last[order[0]]) - 1, int(last[order[1]]) - 1


def build_step_state(num_atoms, t, s, seed):
    """The state a step starts from, float32: frac_coords uniform in [0, 1), lattices 2 I + N(0, 1), atom_types (logits) N(0, 1).
    Every crystal's first coordinate is exactly 0 and its last one exactly nextafter(1, 0); the two hair elements (boundary) are exactly
    0.  (t and s are not needed to write the state; build_noise scales the hair draws by them.)"""
    g = torch.Generator().manual_seed(seed)
    na, _ = _batch(num_atoms)
    B, N = len(na), int(na.sum())
    x = torch.rand(N, 3, generator=g)
    lat = 2 * torch.eye(3) + torch.randn(B, 3, 3, generator=g)
    at = torch.randn(N, NUM_TYPES, generator=g)
    first, last, hc, hp = boundary(na)
    fx = x.view(-1)
    fx[first], fx[last], fx[hc], fx[hp] = 0.0, LAST_BELOW_ONE, 0.0, 0.0
    return dict(frac_coords=x, lattices=lat, atom_types=at, num_atoms=na.clone())


def build_noise(num_atoms, t, s, seed):
    """Standard normal draws (float32) for one step of build_step_state's state, as step's z.  At every crystal's first coordinate the
    corrector's and the predictor's draw are negative, at its last one positive, 0.5 <= |z| <= 3: the sum crosses the cell boundary in
    both halves at every std of the schedule.  hair_corr: corr_x = -HAIR / std_corr, so x_mid is a hair below 0 and pymod1 gives 1.0f.
    hair_pred: corr_x = 0 (x_mid stays exactly 0) and pred_x = -HAIR / std_pred: the predictor's first pymod1 gives 1.0f and its second
    one must fold it to 0.  s: step scalars at t (float64)."""
    g = torch.Generator().manual_seed(seed)
    na, batch = _batch(num_atoms)
    B, N = len(na), int(na.sum())
    z = dict(corr_x=torch.randn(N, 3, generator=g), pred_x=torch.randn(N, 3, generator=g), pred_l=torch.randn(B, 3, 3, generator=g),
             pred_t=torch.randn(N, NUM_TYPES, generator=g))
    first, last, hc, hp = boundary(na)
    for k in ("corr_x", "pred_x"):
        f = z[k].view(-1)
        f[first] = -(0.5 + 2.5 * torch.rand(B, generator=g))
        f[last] = 0.5 + 2.5 * torch.rand(B, generator=g)
    std = lambda k, i: float(s[k][batch[i // 3]])
    z["corr_x"].view(-1)[hc] = -HAIR / std("std_corr", hc)
    z["corr_x"].view(-1)[hp] = 0.0
    z["pred_x"].view(-1)[hp] = -HAIR / std("std_pred", hp)
    return z


# ---- the oracle on the same inputs ------------------------------------------------------------------------------------------------------

def oracle_step(hp, P, tabs, state, z, t, dtype, step_lr=STEP_LR, keep_lattice=False, keep_coords=False):
    """oracle.diffcsp_oracle.sample restricted to the step t -> t - 1 from `state` with the draws z (None at t = 1), every floating-point
    input (state, noise, schedule tables, parameters) taken to `dtype` first.  Returns (traj[t], traj[t - 1]) of the oracle: the first
    holds frac_coords_mid and the three log-probabilities for t > 1, the second the next state."""
    c = lambda v: v.to(dtype)
    sch = O.Schedules(int(t), {k: c(v) for k, v in tabs[0].items()}, {k: c(v) for k, v in tabs[1].items()}, SIGMA_BEGIN, SIGMA_END)
    noise = dict(x_T=c(state["frac_coords"]), l_T=c(state["lattices"]), t_T=c(state["atom_types"]))
    for k in NOISE_KEYS:
        noise[k] = {} if z is None else {int(t): c(z[k])}
    _, traj = O.sample({k: c(v) for k, v in P.items()}, hp, sch, torch.as_tensor(state["num_atoms"]).long(), noise, step_lr=step_lr,
                       t_stop=int(t) - 1, keep_lattice=keep_lattice, keep_coords=keep_coords)
    return traj[int(t)], traj[int(t) - 1]


def network_preds(hp, P, s, state, z, t, dtype, keep_coords=False, freqs=None):
    """step's preds from oracle.diffcsp_oracle.cspnet_forward in `dtype`: the coordinate head at the state, the three heads at the
    corrector's (unwrapped) x_mid, with the time embedding as oracle.diffcsp_oracle.sample forms it (freqs: a pinned frequency table)."""
    c = lambda v: v.to(dtype)
    na, batch = _batch(state["num_atoms"])
    Pd = {k: c(v) for k, v in P.items()}
    times = torch.full((len(na),), int(t))
    temb = O.time_embedding(times, hp.time_dim) if freqs is None else torch.cat(((times[:, None] * freqs[None, :]).sin(),
                                                                                  (times[:, None] * freqs[None, :]).cos()), dim=-1)
    x, lat, at = c(state["frac_coords"]), c(state["lattices"]), c(state["atom_types"])
    net = lambda xx: O.cspnet_forward(Pd, hp, temb, at, xx, lat, na, batch)
    _, px_c, _ = net(x)
    sd = {k: c(v) for k, v in s.items()}
    _, xm = corrector(sd, x, px_c, None if z is None else c(z["corr_x"]), na, keep_coords)
    pl, px_p, pt = net(xm)
    return px_c, pl, px_p, pt

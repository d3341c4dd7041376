"""Float64 restatement of the trajectory likelihood of a CONDITIONED chain (include/matinvent_hip_lik.h): the three
log-probabilities of a recorded step, their local derivatives and the per-step transition KL, with the predictor terms of the known
elements left out and the divisors kept.  Built on tests/traj_ref64.py's functions (wrapped_normal, _normal, _crystal_mean, kl), which
it imports; with all-false masks every function here IS the unmasked reference.

masks = (known_types [N], known_coords [N], known_lattice [B]), bool.  Per crystal of n atoms:
    lp_l = 0 where known_lattice, else the mean over the 9 entries
    lp_t = sum over atoms with known_types == 0 of the per-atom mean over the 100 logits, / n
    lp_x = corrector mean over all 3 n coordinates + sum over atoms with known_coords == 0 of the predictor terms, / 3 / n
and the same for the KL's predictor terms; dl, dt, dx_pred are 0 at masked elements, dx_corr is untouched.

Also here: `formulas32`, the same quantities as the separately rounded tensor ops of tests/traj_util.py (the oracle's naive 21-image
sum, torch means) in a chosen dtype -- in float32 the yardstick of the device's rounding, as tests/test_gpu_traj_arithmetic.py takes
it -- and `elementwise`, plain Python loops over crystals, atoms and entries, against which the vectorised forms are checked.
Plain torch / math, CPU; shared by the CPU and the GPU tests."""
import math

import torch

from oracle import diffcsp_oracle as O
from tests import traj_ref64 as R

NUM_TYPES = R.NUM_TYPES


def _free(masks, dtype):
    kt, kx, kl = (torch.as_tensor(m).bool() for m in masks)
    return (~kt).to(dtype), (~kx).to(dtype), (~kl).to(dtype)


def logprobs(s, state, preds, masks):
    """traj_ref64.logprobs under `masks`: (lp_l, lp_t, lp_x) [B] and (dl [B,3,3], dt [N,100], dx_corr [N,3], dx_pred [N,3])."""
    px_c, pl, px_p, pt = preds
    ft, fx, fl = _free(masks, torch.float64)
    na, batch = R._batch(state["num_atoms"])
    n = na.clamp(min=1).double()[batch][:, None]
    pa = lambda k: s[k][batch][:, None]
    pb = lambda k: s[k][:, None, None]
    x, xm = state["frac_coords"], state["frac_coords_mid"]
    kc, kp = pa("step_corr") * pa("sqrt_sn"), pa("step_pred") * pa("sqrt_sn")
    lc, dc = R.wrapped_normal(xm, (x - kc * px_c) % 1.0, pa("std_corr"))
    lq, dq = R.wrapped_normal(state["next_frac_coords"], (xm - kp * px_p) % 1.0, pa("std_pred"))
    lp_x = R._crystal_mean(lc.mean(dim=-1), batch, na) + R._crystal_mean(lq.mean(dim=-1) * fx, batch, na)
    ll, dl = R._normal(state["next_lattices"], pb("c0") * (state["lattices"] - pb("c1") * pl), pb("sigma"))
    lt, dt = R._normal(state["next_atom_types"], pa("c0") * (state["atom_types"] - pa("c1") * pt), pa("sigma"))
    lp_l = ll.mean(dim=(-1, -2)) * fl
    lp_t = R._crystal_mean(lt.mean(dim=-1) * ft, batch, na)
    d = (dl * -(pb("c0") * pb("c1")) / 9 * fl[:, None, None], dt * -(pa("c0") * pa("c1")) / (NUM_TYPES * n) * ft[:, None],
         dc * -kc / (3 * n), dq * -kp / (3 * n) * fx[:, None])
    return (lp_l, lp_t, lp_x), tuple(v.detach() for v in d)


def kl(s, num_atoms, preds_agent, preds_prior, masks):
    """traj_ref64.kl under `masks`: (kl_l, kl_t, kl_x) [B] and the derivatives with respect to the agent's (pl, pt, px_corr, px_pred)."""
    ft, fx, fl = _free(masks, torch.float64)
    na, batch = R._batch(num_atoms)
    n = na.clamp(min=1).double()[batch][:, None]
    pa = lambda k: s[k][batch][:, None]
    cc, var = s["c0"] * s["c1"], s["sigma"] ** 2
    (xc_a, l_a, xp_a, t_a), (xc_p, l_p, xp_p, t_p) = preds_agent, preds_prior
    ml = cc[:, None, None] * (l_a - l_p)
    mt = cc[batch][:, None] * (t_a - t_p)
    kl_l = (ml ** 2).mean(dim=(-1, -2)) / (2 * var) * fl
    kl_t = R._crystal_mean((mt ** 2).mean(dim=-1) * ft, batch, na) / (2 * var)
    d = [ml * (cc / var)[:, None, None] / 9 * fl[:, None, None], mt * (cc / var)[batch][:, None] / (NUM_TYPES * n) * ft[:, None]]
    kl_x = 0
    for step, std, a, p, keep in (("step_corr", "std_corr", xc_a, xc_p, torch.ones_like(fx)), ("step_pred", "std_pred", xp_a, xp_p, fx)):
        k = pa(step) * pa("sqrt_sn")
        m = k * (a - p)
        m = m - torch.round(m)
        kl_x = kl_x + R._crystal_mean((m ** 2 / (2 * pa(std) ** 2)).mean(dim=-1) * keep, batch, na)
        d.append(m * k / pa(std) ** 2 / (3 * n) * keep[:, None])
    return (kl_l, kl_t, kl_x), tuple(v.detach() for v in d)


def formulas32(s, state, preds, masks, dtype=torch.float32):
    """(lp_l, lp_t, lp_x) as the separately rounded tensor ops of tests/traj_util.forward_logprb in `dtype` (s: kl_util.step_scalars in
    that dtype; state, preds cast here), with the masked terms multiplied out before the crystal's mean.  Differentiable with respect to
    preds."""
    c = lambda v: v.to(dtype) if v.is_floating_point() else v
    px_c, pl, px_p, pt = (c(v) for v in preds)
    st = {k: c(v) for k, v in state.items()}
    ft, fx, fl = _free(masks, dtype)
    na, batch = R._batch(st["num_atoms"])
    B = len(na)
    pa = lambda k: s[k][batch][:, None]
    pb = lambda k: s[k][:, None, None]
    x, xm = st["frac_coords"], st["frac_coords_mid"]
    mu = (x - pa("step_corr") * (px_c * pa("sqrt_sn"))) % 1.0
    lp_xc = O.scatter_mean(O.log_prob_wn(xm, mu, pa("std_corr")).mean(dim=-1), batch, B)
    mu = (xm - pa("step_pred") * (px_p * pa("sqrt_sn"))) % 1.0
    lp_xp = O.scatter_mean(O.log_prob_wn(st["next_frac_coords"], mu, pa("std_pred")).mean(dim=-1) * fx, batch, B)
    lp_l = O.normal_log_prob(st["next_lattices"], pb("c0") * (st["lattices"] - pb("c1") * pl), pb("sigma")).mean(dim=-1).mean(dim=-1) * fl
    lp_t = O.scatter_mean(O.normal_log_prob(st["next_atom_types"], pa("c0") * (st["atom_types"] - pa("c1") * pt), pa("sigma")).mean(dim=-1) * ft,
                          batch, B)
    return lp_l, lp_t, lp_xc + lp_xp


def kl32(s, num_atoms, preds_agent, preds_prior, masks, dtype=torch.float32):
    """(kl_l, kl_t, kl_x) as tests/kl_util.kl_terms forms them, in `dtype`, with the masked predictor terms multiplied out."""
    from tests.kl_util import min_image
    ft, fx, fl = _free(masks, dtype)
    na, batch = R._batch(num_atoms)
    B = len(na)
    (xc_a, l_a, xp_a, t_a), (xc_p, l_p, xp_p, t_p) = ([v.to(dtype) for v in p] for p in (preds_agent, preds_prior))
    cc, var = s["c0"] * s["c1"], s["sigma"] ** 2
    dl = cc[:, None, None] * (l_a - l_p)
    kl_l = (dl ** 2 / (2 * var[:, None, None])).mean(dim=(-1, -2)) * fl
    dt = cc[batch][:, None] * (t_a - t_p)
    kl_t = O.scatter_mean((dt ** 2 / (2 * var[batch][:, None])).mean(dim=-1) * ft, batch, B)
    kl_x = 0
    for step, std, a, p, keep in (("step_corr", "std_corr", xc_a, xc_p, torch.ones_like(fx)), ("step_pred", "std_pred", xp_a, xp_p, fx)):
        k = (s[step] * s["sqrt_sn"])[batch][:, None]
        d = min_image(k * (a - p))
        kl_x = kl_x + O.scatter_mean((d ** 2 / (2 * s[std][batch][:, None] ** 2)).mean(dim=-1) * keep, batch, B)
    return kl_l, kl_t, kl_x


def elementwise(s, state, preds, masks):
    """(lp_l, lp_t, lp_x) as nested Python lists by explicit loops over crystals, atoms, coordinates and logits (math, float64): the
    definition of DESIGN 36 spelled out, with no masking by multiplication and no tensor reductions."""
    px_c, pl, px_p, pt = (v.double() for v in preds)
    kt, kx, kl = (torch.as_tensor(m).bool().tolist() for m in masks)
    na = [int(v) for v in state["num_atoms"]]
    sc = {k: v.double().tolist() for k, v in s.items()}

    def wn(x, mu, std):
        return math.log(sum(math.exp(-(x - mu + k) ** 2 / (2 * std ** 2)) for k in range(-10, 11)))

    def normal(v, m, sigma):
        return -(v - m) ** 2 / (2 * sigma ** 2) - math.log(sigma) - 0.5 * math.log(2 * math.pi)

    x, xm, xn = (state[k].double().tolist() for k in ("frac_coords", "frac_coords_mid", "next_frac_coords"))
    lat, latn = state["lattices"].double().reshape(-1, 9).tolist(), state["next_lattices"].double().reshape(-1, 9).tolist()
    at, atn = state["atom_types"].double().tolist(), state["next_atom_types"].double().tolist()
    pxc, pxp, ptl, pll = px_c.tolist(), px_p.tolist(), pt.tolist(), pl.reshape(-1, 9).tolist()
    out_l, out_t, out_x = [], [], []
    i0 = 0
    for b, n in enumerate(na):
        c0, c1, sig = sc["c0"][b], sc["c1"][b], sc["sigma"][b]
        kc, kp = sc["step_corr"][b] * sc["sqrt_sn"][b], sc["step_pred"][b] * sc["sqrt_sn"][b]
        out_l.append(0.0 if kl[b] else sum(normal(latn[b][j], c0 * (lat[b][j] - c1 * pll[b][j]), sig) for j in range(9)) / 9)
        lt = lc = lq = 0.0
        for i in range(i0, i0 + n):
            if not kt[i]:
                lt += sum(normal(atn[i][k], c0 * (at[i][k] - c1 * ptl[i][k]), sig) for k in range(NUM_TYPES)) / NUM_TYPES
            for j in range(3):
                lc += wn(xm[i][j], (x[i][j] - kc * pxc[i][j]) % 1.0, sc["std_corr"][b])
                if not kx[i]:
                    lq += wn(xn[i][j], (xm[i][j] - kp * pxp[i][j]) % 1.0, sc["std_pred"][b])
        out_t.append(lt / max(n, 1))
        out_x.append(lc / 3 / max(n, 1) + lq / 3 / max(n, 1))
        i0 += n
    return out_l, out_t, out_x


def masks_of(cond):
    """(known_types, known_coords, known_lattice) of a conditioning.Condition."""
    return cond.known_types, cond.known_coords, cond.known_lattice


def make_masks(num_atoms, mode, seed=0):
    """all / none / mixed (per atom, types and coordinates drawn independently; per crystal for the lattice; every crystal of two atoms
    or more gets at least one free and one known atom in each part where the draw allows, crystal 0's lattice known and crystal 1's free)."""
    na = [int(v) for v in num_atoms]
    B, N = len(na), sum(na)
    if mode in ("all", "none"):
        v = mode == "all"
        return torch.full((N,), v), torch.full((N,), v), torch.full((B,), v)
    g = torch.Generator().manual_seed(seed)
    kt, kx, kl = torch.rand(N, generator=g) < 0.5, torch.rand(N, generator=g) < 0.5, torch.rand(B, generator=g) < 0.5
    kl[0] = True
    if B > 1:
        kl[1] = False
    i0 = 0
    for n in na:
        if n >= 2:
            kt[i0], kt[i0 + 1] = True, False
            kx[i0], kx[i0 + 1] = False, True
        i0 += n
    return kt, kx, kl

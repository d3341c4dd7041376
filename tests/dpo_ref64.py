"""Float64 reference of the preference (Diffusion-DPO) micro-step's own arithmetic (matinvent_amd/csrc/dpo.hip: dpo_delta_kernel,
dpo_pair_kernel, dpo_seed_kernel; include/matinvent_hip_dpo.h states the formulas) with no device code in it, built on tests/ft_ref64.py
for the sets, the noise, add_noise, zero_head_preds and the oracle micro-step.  Every function takes the predictions as an argument and a
`dtype` (float64: the reference; float32: the same separately rounded formulas, the yardstick of the device's tolerance), and is
differentiable torch.  oracle_dpo_micro_step / oracle_dpo_step restate one micro-step / the whole step with oracle.diffcsp_oracle forwards,
torch autograd and torch.optim.Adam.  Plain torch, CPU; shared by the CPU and the GPU tests."""
import torch

from oracle import diffcsp_oracle as O
from tests import ft_ref64 as R

NUM_TYPES = R.NUM_TYPES
COSTS = R.COSTS


def _weighted(fl, fx, ft, costs, num_atoms):
    """cl mean9(fl) + cx mean_i mean3(fx) + ct mean_i mean100(ft) per crystal, for per-element terms fl [B,3,3], fx [N,3], ft [N,100]."""
    na, n2g = R._batch(num_atoms)
    m = lambda v: R._crystal_mean(v.mean(dim=-1), n2g, na)
    return costs[0] * fl.mean(dim=(-1, -2)) + costs[1] * m(fx) + costs[2] * m(ft)


def sample_loss(preds, targets, costs, num_atoms, dtype=torch.float64):
    """L_b = cl mean9((pl - rl)^2) + cx mean_i mean3((px - tx)^2) + ct mean_i mean100((pt - rt)^2)."""
    (pl, px, pt), (rl, tx, rt) = ([v.to(dtype) for v in g] for g in (preds, targets))
    return _weighted((pl - rl) ** 2, (px - tx) ** 2, (pt - rt) ** 2, costs, num_atoms)


def delta(preds_agent, preds_prior, targets, costs, num_atoms, dtype=torch.float64):
    """d_b = L_b(agent) - L_b(prior) in the FACTORISED form: the weighted means of (pa - pp)(pa + pp - 2 target) per element."""
    (pl, px, pt), (ql, qx, qt), (rl, tx, rt) = ([v.to(dtype) for v in g] for g in (preds_agent, preds_prior, targets))
    f = lambda a, p, t: (a - p) * (a + p - 2 * t)
    return _weighted(f(pl, ql, rl), f(px, qx, tx), f(pt, qt, rt), costs, num_atoms)


def delta_direct(preds_agent, preds_prior, targets, costs, num_atoms, dtype=torch.float64):
    """d_b as the difference of the two reduced losses: what the device must NOT compute (it cancels at agent ~ prior in float32)."""
    return sample_loss(preds_agent, targets, costs, num_atoms, dtype) - sample_loss(preds_prior, targets, costs, num_atoms, dtype)


def pair_terms(d, pairs, beta):
    """(m, u, loss, g) per pair (w, l) of `pairs` [P, 2]: m = d_w - d_l, u = beta m, loss = softplus(u) = -log sigmoid(-u), g = sigmoid(u).
    logaddexp / sigmoid: exact and finite for any finite u."""
    pairs = torch.as_tensor(pairs).long().reshape(-1, 2)
    m = d[pairs[:, 0]] - d[pairs[:, 1]]
    u = beta * m
    return m, u, torch.logaddexp(u, torch.zeros_like(u)), torch.sigmoid(u)


def coefficients(g, pairs, B, beta, p_global, accum):
    """c_b = beta / (p_global accum) (sum_{p: w_p = b} g_p - sum_{p: l_p = b} g_p); 0 for a crystal in no pair."""
    pairs = torch.as_tensor(pairs).long().reshape(-1, 2)
    c = torch.zeros(B, dtype=g.dtype).index_add(0, pairs[:, 0], g).index_add(0, pairs[:, 1], -g)
    return c * beta / (p_global * accum)


def seeds(preds_agent, targets, costs, num_atoms, coef, dtype=torch.float64):
    """d total / d (pl, px, pt) of total = sum_p loss_p / (p_global accum) in closed form, from the crystals' coefficients c_b:
    c_b cl 2 (pl - rl) / 9, c_b cx 2 (px - tx) / (3 n_b), c_b ct 2 (pt - rt) / (100 n_b)."""
    na, n2g = R._batch(num_atoms)
    (pl, px, pt), (rl, tx, rt) = ([v.to(dtype) for v in g] for g in (preds_agent, targets))
    c = coef.to(dtype)
    n = na.clamp(min=1).to(dtype)[n2g][:, None]
    a = c[n2g][:, None]
    return (c[:, None, None] * costs[0] * 2 * (pl - rl) / 9, a * costs[1] * 2 * (px - tx) / (3 * n), a * costs[2] * 2 * (pt - rt) / (NUM_TYPES * n))


def stats(m, loss, p_global):
    """What one micro-step adds to the three statistics rows: sum_p loss_p / p_global, #{p : m_p < 0}, sum_p (-m_p)."""
    return torch.stack([loss.sum() / p_global, (m < 0).to(m.dtype).sum(), (-m).sum()])


def total(preds_agent, preds_prior, targets, costs, num_atoms, pairs, beta, p_global, accum, dtype=torch.float64):
    """sum_p softplus(beta (d_w - d_l)) / (p_global accum), differentiable in the agent's predictions."""
    d = delta(preds_agent, preds_prior, targets, costs, num_atoms, dtype)
    return pair_terms(d, pairs, beta)[2].sum() / (p_global * accum)


def micro_step(preds_agent, preds_prior, targets, costs, num_atoms, pairs, beta, p_global, accum, dtype=torch.float64):
    """Everything the loss stage produces from given predictions: dict(L, delta, m, u, loss, g, coef, seeds, stats)."""
    B = len(torch.as_tensor(num_atoms))
    d = delta(preds_agent, preds_prior, targets, costs, num_atoms, dtype)
    m, u, loss, g = pair_terms(d, pairs, beta)
    coef = coefficients(g, pairs, B, beta, p_global, accum)
    return dict(L=sample_loss(preds_agent, targets, costs, num_atoms, dtype), delta=d, m=m, u=u, loss=loss, g=g, coef=coef,
                seeds=seeds(preds_agent, targets, costs, num_atoms, coef, dtype), stats=stats(m, loss, p_global))


# ---- the oracle on the same inputs --------------------------------------------------------------------------------------------------

def oracle_dpo_micro_step(hp, P, Q, tables, fs, nz, dtype, pairs, beta, time_idx, p_global, accum=1, costs=COSTS, freqs=None, grad=False):
    """One preference micro-step through oracle.diffcsp_oracle on the CPU with every floating-point input taken to `dtype` first
    (ft_ref64.oracle_micro_step's conventions): add_noise at `time_idx`, calc_sample_loss of both networks for the predictions, the
    factorised d_b, total = sum_p softplus(beta (d_w - d_l)) / (p_global accum).  Returns dict(preds, prior_preds, targets, delta, m, loss,
    stats (as the step accumulates them), grads = {name: d total / d P[name]} with grad=True)."""
    c = lambda v: v.to(dtype) if v.is_floating_point() else v
    timesteps = len(tables["alphas_cumprod"]) - 1
    noised = R.oracle_add_noise(tables, fs, nz, dtype, time_idx)
    B = len(fs["num_atoms"])
    t = torch.full((B,), timesteps - int(time_idx))
    t_emb = c(noised[0][0]) if freqs is None else R.time_embedding(t, c(freqs))
    noised = ((t_emb,) + tuple(noised[0][1:]), noised[1], noised[2])
    Pg = {k: c(v).detach().clone().requires_grad_(grad) for k, v in P.items()}
    _, pa = O.calc_sample_loss(Pg, hp, O.Costs(*costs), noised)
    with torch.no_grad():
        _, pp = O.calc_sample_loss({k: c(v) for k, v in Q.items()}, hp, O.Costs(*costs), noised)
    d = delta(pa, pp, noised[1], costs, fs["num_atoms"], dtype)
    m, u, loss, g = pair_terms(d, pairs, beta)
    tot = loss.sum() / (p_global * accum)
    out = dict(preds=tuple(v.detach() for v in pa), prior_preds=tuple(pp), targets=noised[1], delta=d.detach(), m=m.detach(), loss=loss.detach(),
               stats=stats(m, loss, p_global).detach())
    if grad:
        names = list(Pg)
        out["grads"] = dict(zip(names, torch.autograd.grad(tot, [Pg[k] for k in names], allow_unused=True)))
    return out


def oracle_dpo_step(agent, prior, hp, sch, costs, batch, pairs, noise_fn, *, lr, timesteps, accum_steps, beta, epochs=1, record=None):
    """preference.dpo_step restated: the loop of oracle.diffcsp_oracle.ft_step (one batch holding the set, `noise_fn(epoch, t)` ->
    dict(rand_l, rand_x, rand_t), an optimizer step wherever an accumulation window closes, a fresh Adam per call) with the loss
    sum_p softplus(beta (d_w - d_l)) / (P accum_steps), torch autograd and torch.optim.Adam.  Updates `agent` in place; `record` collects
    per-micro-step loss (sum_p loss_p / P) and m."""
    P = len(pairs)
    params = [p.requires_grad_(True) for p in agent.values()]
    opt = torch.optim.Adam(params, lr=lr)
    for epoch in range(epochs):
        opt.zero_grad(set_to_none=False)
        t = -1
        for t in range(timesteps):
            noised = O.add_noise(hp, sch, batch, t, noise_fn(epoch, t))
            _, pa = O.calc_sample_loss(agent, hp, costs, noised)
            with torch.no_grad():
                _, pp = O.calc_sample_loss(prior, hp, costs, noised)
            d = delta(pa, pp, noised[1], (costs.lattice, costs.coord, costs.type), batch["num_atoms"], pa[0].dtype)
            m, _, loss, _ = pair_terms(d, pairs, beta)
            (loss.sum() / (P * accum_steps)).backward()
            if record is not None:
                record.setdefault("loss", []).append((loss.sum() / P).detach().clone())
                record.setdefault("m", []).append(m.detach().clone())
            if (t + 1) % accum_steps == 0:
                opt.step()
                opt.zero_grad(set_to_none=False)
        if (t + 1) % accum_steps != 0:
            opt.step()
    for p in params:
        p.requires_grad_(False)
    return agent

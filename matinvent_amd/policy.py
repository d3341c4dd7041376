"""PPO-clipped policy gradient on recorded reverse-diffusion trajectories (DDPO-style), the log-probability objective next to
MatInvent's reward-weighted denoising loss (finetune.ft_step).

For every kept crystal b of a rollout (sampling.sample_rollout) and a diffusion time t drawn from 2..T, the step t -> t-1 is
re-evaluated under the current weights (DiffCSPModule.forward_logprb's arithmetic):

    lp_new = w . (log_prob_l, log_prob_t, log_prob_x),  lp_old = w . (the sampler's record),  rho = exp(lp_new - lp_old)
    L_b    = max(-A_b rho, -A_b clip(rho, 1 - eps, 1 + eps)),      loss = sum over micro-steps and crystals of L_b / M

with A the normalised, clipped advantages and M = B * accum_steps (ft_step's `/ accum_steps` convention).  Each micro-step is ONE C
call (mi_traj_pg_step: gather, two taped evaluations, surrogate and seeds, backward into theta.grad) with no host synchronisation;
the statistics are read back once per epoch.

With kl_coef = beta > 0 every crystal's term becomes L_b + beta KL_b, KL_b = w . (KL_l, KL_t, KL_x) the closed-form KL of the agent's
transition p_theta(x_{t-1} | x_t) from the frozen prior's at the same step (DPOK's per-step regulariser), one
mi_traj_pg_kl_step per micro-step."""
import ctypes as C
import logging

import numpy as np
import torch

from . import _lib
from .cspnet import _ptr, _stream
from .optim import FusedAdam, cfg_get, clip_options, epoch_grad_stats, window_closes

# clip_range: DDPO's 1e-4 is below the rounding of the re-evaluated lattice log-probability -- at unchanged weights |log rho| reaches 0.12 over a
# T = 1000 chain of the benchmark network -- so the default is PPO's 0.2, above that measured maximum
DEFAULTS = dict(clip_range=0.2, adv_clip=5.0, logprob_weights=(1.0, 1.0, 1.0), kl_coef=0.0)
# kl_coef > 0: the prior's two inference evaluations of a micro-step on an auxiliary stream, overlapping the agent's -- the same bits as
# serial; the added cost per micro-step falls from 2.0 to 1.1 ms at 64 crystals, from 5.2 to 4.3 ms at 256
PG_KL_AUX = True


def advantages(rewards, adv_clip=DEFAULTS["adv_clip"]):
    """(r - mean) / (std + 1e-8) with the population std, clipped to +-adv_clip; float32 [B] (host)."""
    r = np.asarray(rewards, dtype=np.float64)
    a = (r - r.mean()) / (r.std() + 1e-8)
    return np.clip(a, -adv_clip, adv_clip).astype(np.float32)


def draw_timesteps(T, B, timesteps, epochs, seed=None):
    """For each epoch and each crystal, `timesteps` distinct times from 2..T without replacement (capped at T - 1, all of them), from a
    generator seeded with `seed`.  Returns a list of `epochs` int32 arrays [K, B]: row k holds every crystal's time of micro-step k."""
    K = min(int(timesteps), T - 1)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(epochs):
        perm = np.argsort(rng.random((B, T - 1)), axis=1)[:, :K] + 2      # a uniform K-subset of 2..T per crystal, in random order
        out.append(np.ascontiguousarray(perm.T.astype(np.int32)))
    return out


def pg_step(agent, rollout, rewards, cfg, seed=None, log=logging.info, prior=None):
    """One call of the PPO-clipped policy gradient over every crystal of `rollout` (sampling.Rollout) with rewards [B].

    cfg (finetune_cfg; key or attribute access): lr, epochs, timesteps (draws per crystal per epoch, capped at T - 1), accum_steps
    (micro-steps per optimiser step; a partial window at the end of an epoch steps too), clip_range (eps, default 0.2), adv_clip
    (default 5.0), logprob_weights (w, default [1, 1, 1]), kl_coef (beta, default 0; > 0 needs `prior`, the frozen DiffCSPModule whose
    transitions anchor the agent's).  Micro-step k evaluates every crystal at its k-th draw, so one pair of batch handles (and one
    handle of the prior) serves the call; they are released on return.  A fresh FusedAdam per call, like ft_step.  `seed` seeds the
    timestep draws.  Returns one dict per epoch: loss (mean of L_b over micro-steps and crystals: the clipped surrogate alone), ratio_mean,
    approx_kl (mean of (lp_new - lp_old)^2 / 2) and clip_frac (fraction with |rho - 1| > eps); with kl_coef > 0 also prior_kl (mean of
    KL_b).  kl_coef = 0 is the surrogate alone: the prior is not evaluated.
    max_grad_norm (a number > 0) clips every optimiser step's gradient to that global norm (DDPO's / DPOK's max_grad_norm) and
    skip_nonfinite_steps (bool) leaves out a step whose gradient holds inf / NaN, both on the device inside FusedAdam.step;
    with either, the dicts also carry grad_norm (mean norm before clipping), grad_norm_max, clipped_steps and skipped_steps of the epoch,
    read in the same transfer as the rest.
    A strided chain: `agent` a view made by DiffCSPModule.respaced and `rollout` recorded through it -- T is then the view's S,
    the draws come from 2..S and every time is a step index; with kl_coef > 0 `prior` must be a view on the same grid.  The optimiser
    steps land in the view's base module: they share theta.
    A conditioned rollout: when rollout.condition is set (sample_rollout(..., condition=c, likelihood="free")) the call's
    handles -- the agent pair and, with kl_coef > 0, the prior's -- carry its masks as their likelihood mask from before the first
    micro-step until the return: log-probabilities, KL terms and gradients leave out the predictor terms of the known elements."""
    opt = clip_options(cfg)
    from .guidance import refuse_latent
    refuse_latent((agent, prior), "pg_step")
    lr, epochs = float(cfg_get(cfg, "lr")), int(cfg_get(cfg, "epochs"))
    timesteps, accum_steps = int(cfg_get(cfg, "timesteps")), int(cfg_get(cfg, "accum_steps"))
    clip_range = float(cfg_get(cfg, "clip_range", DEFAULTS["clip_range"]))
    adv_clip = float(cfg_get(cfg, "adv_clip", DEFAULTS["adv_clip"]))
    w = [float(v) for v in cfg_get(cfg, "logprob_weights", DEFAULTS["logprob_weights"])]
    if len(w) != 3:
        raise ValueError(f"pg_step: logprob_weights needs three values (l, t, x), got {w}")
    kl_coef = float(cfg_get(cfg, "kl_coef", DEFAULTS["kl_coef"]))
    if not kl_coef >= 0.0:
        raise ValueError(f"pg_step: kl_coef = {kl_coef}: must be >= 0")
    if kl_coef > 0.0 and prior is None:
        raise ValueError(f"pg_step: kl_coef = {kl_coef} > 0 needs the frozen prior (prior=None)")
    if accum_steps < 1 or epochs < 0 or timesteps < 1:
        raise ValueError(f"pg_step: accum_steps = {accum_steps}, epochs = {epochs}, timesteps = {timesteps}")
    B, T = rollout.num_graphs, rollout.T
    if len(rewards) != B:
        raise ValueError(f"pg_step: {len(rewards)} rewards for {B} crystals")
    if B == 0:
        raise ValueError("pg_step: the rollout holds no crystal")
    if T != agent.beta_scheduler.timesteps:
        raise ValueError(f"pg_step: the rollout's chain has T = {T}, the agent's T = {agent.beta_scheduler.timesteps}")
    if kl_coef > 0.0 and not _same_time_map(agent, prior):
        raise ValueError("pg_step: the prior's time map differs from the agent's: a strided agent (DiffCSPModule.respaced) needs the prior "
                         "re-spaced to the same grid, prior=prior.respaced(times=agent.time_map)")
    dev = agent.device
    dec = agent.decoder
    theta = dec.theta
    adv = torch.from_numpy(advantages(rewards, adv_clip)).to(dev)                 # one upload per call
    draws = draw_timesteps(T, B, timesteps, epochs, seed)
    K = draws[0].shape[0] if draws else 0
    M = B * accum_steps
    na = [int(v) for v in rollout.num_atoms.tolist()]
    b_corr, b_pred = agent.make_batch(na), agent.make_batch(na)                    # this call's pair (freed with the objects on return)
    use_kl = kl_coef > 0.0
    b_prior = prior.make_batch(na) if use_kl else None                             # (a strided view's handles carry its time map)
    aux = None
    if use_kl and PG_KL_AUX:
        from .streams import concurrent_streams
        aux = concurrent_streams(2, dev)[1]
        if aux == torch.cuda.current_stream():
            aux = concurrent_streams(2, dev)[0]
    w_host = np.asarray(w, dtype=np.float32)
    optimizer = FusedAdam([theta], lr=lr, **opt)
    if theta.grad is None:
        theta.grad = torch.zeros_like(theta)
    stats = torch.zeros(5 if use_kl else 4, B, device=dev)
    handles = (b_corr, b_pred)
    cond = getattr(rollout, "condition", None)
    if cond is not None:                                                           # fresh handles, nothing in flight on them: blocking copies, once per call
        for cb in handles + ((b_prior,) if use_kl else ()):
            cond.attach_likelihood(agent, cb)
    if use_kl:                                                                     # the micro-step of this call, chosen once
        micro_step = lambda th, td: pg_kl_micro_step(agent, handles, prior, b_prior, rollout, th, td, adv, clip_range, w_host, kl_coef, 1.0 / M,
                                                     theta.grad, stats, aux_stream=aux)
    else:
        micro_step = lambda th, td: pg_micro_step(agent, handles, rollout, th, td, adv, clip_range, w_host, 1.0 / M, theta.grad, stats)
    out = []
    for epoch in range(epochs):
        agent.train()
        optimizer.zero_grad(set_to_none=False)
        stats.zero_()
        t_host = draws[epoch]
        t_dev = torch.from_numpy(t_host).to(dev)                                   # one upload per epoch: [K, B]
        for k in range(K):
            micro_step(t_host[k], t_dev[k])
            if window_closes(k + 1, accum_steps, K):
                optimizer.step()
                optimizer.zero_grad(set_to_none=False)
        s = stats.sum(dim=1) / max(1, K * B)
        if optimizer.guarded:                                                      # (the optimiser's statistics ride in the same transfer)
            s = torch.cat([s.double(), optimizer.grad_stats(reset=True)])
        s = s.tolist()                                                             # one read-back per epoch
        d = dict(loss=s[0], ratio_mean=s[1], approx_kl=s[2], clip_frac=s[3])
        if use_kl:
            d["prior_kl"] = s[4]
        if optimizer.guarded:
            d.update(epoch_grad_stats(s[stats.shape[0]:]))
        out.append(d)
        log(f"PG epoch {epoch}: " + ", ".join(f"{k}: {v:.4g}" for k, v in d.items()))
    del b_corr, b_pred, b_prior, handles, micro_step
    return out


def _same_time_map(a, b):
    """Both modules on their trained grids, or both strided views (DiffCSPModule.respaced) of one grid."""
    ta, tb = getattr(a, "time_map", None), getattr(b, "time_map", None)
    if ta is None or tb is None:
        return ta is None and tb is None
    return ta.tolist() == tb.tolist()


def _micro_step_args(agent, rollout, t_host, t_dev, w_host):
    """What both micro-steps check and marshal: the rollout's five arrays (device, float32, contiguous), t_host / w_host as contiguous
    int32 [B] / float32 [3] with their shapes checked; ends with the agent's decoder.sync().  Returns (traj, t_host, w_host)."""
    traj = [rollout.atom_types, rollout.frac_coords, rollout.frac_coords_mid, rollout.lattices, rollout.lp_old]
    for v in traj:
        assert v.is_cuda and v.dtype == torch.float32 and v.is_contiguous()
    t_host = np.ascontiguousarray(t_host, dtype=np.int32)
    w_host = np.ascontiguousarray(w_host, dtype=np.float32)
    assert t_host.shape == (rollout.num_graphs,) and w_host.shape == (3,) and t_dev.dtype == torch.int32
    agent.decoder.sync()
    return traj, t_host, w_host


def pg_micro_step(agent, handles, rollout, t_host, t_dev, adv, clip_range, w_host, loss_scale, grad, stats, log_prob=None):
    """One mi_traj_pg_step: every crystal of `rollout` at its time t_host[b] (int32 host [B]; t_dev the same on the device), advantages
    adv [B] (device), weights w_host (float32 host [3]); grad += the surrogate's gradient scaled by loss_scale, stats [4, B] += (L_b, rho,
    approx-KL term, clipped indicator); log_prob [3, B] (optional) receives the new log-probabilities.  `handles`: two batch handles of
    agent.decoder over rollout.num_atoms.  Enqueued on the current stream without a host synchronisation."""
    traj, t_host, w_host = _micro_step_args(agent, rollout, t_host, t_dev, w_host)
    _lib.check(_lib.load().mi_traj_pg_step(agent.decoder._h, handles[0]._h, handles[1]._h, _ptr(agent._coefficients_dev(rollout.step_lr)),
                                           rollout.T, _ptr(agent.time_embedding.freqs), *(_ptr(v) for v in traj), t_host.ctypes.data,
                                           _ptr(t_dev), _ptr(adv), float(clip_range), w_host.ctypes.data, float(loss_scale), _ptr(log_prob),
                                           _ptr(grad), _ptr(stats), _stream()), "mi_traj_pg_step")


def pg_kl_micro_step(agent, handles, prior, prior_handle, rollout, t_host, t_dev, adv, clip_range, w_host, kl_coef, loss_scale, grad, stats,
                     log_prob=None, kl_out=None, aux_stream=None):
    """One mi_traj_pg_kl_step: pg_micro_step's arguments plus the frozen `prior` (a DiffCSPModule; prior_handle: one batch handle of
    prior.decoder over rollout.num_atoms) and kl_coef (beta >= 0).  grad += the gradient of (L_b + beta KL_b) scaled by loss_scale; stats
    [5, B]: rows 0..3 as pg_micro_step's, row 4 += KL_b (weighted by w, not by beta); kl_out [3, B] (optional) receives (KL_l, KL_t, KL_x).
    aux_stream (a torch stream, optional): the prior's evaluations run on it.  Enqueued on the current stream without a host
    synchronisation."""
    assert stats.shape == (5, rollout.num_graphs)
    traj, t_host, w_host = _micro_step_args(agent, rollout, t_host, t_dev, w_host)
    prior.decoder.sync()
    aux = C.c_void_p(aux_stream.cuda_stream) if aux_stream is not None else None
    _lib.check(_lib.load().mi_traj_pg_kl_step(agent.decoder._h, handles[0]._h, handles[1]._h, prior.decoder._h, prior_handle._h,
                                              _ptr(agent._coefficients_dev(rollout.step_lr)), rollout.T, _ptr(agent.time_embedding.freqs),
                                              *(_ptr(v) for v in traj), t_host.ctypes.data, _ptr(t_dev), _ptr(adv), float(clip_range),
                                              w_host.ctypes.data, float(loss_scale), float(kl_coef), _ptr(log_prob), _ptr(kl_out), _ptr(grad),
                                              _ptr(stats), _stream(), aux), "mi_traj_pg_kl_step")

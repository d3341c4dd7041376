"""The preference fine-tune on ranked pairs of FINAL crystals (Diffusion-DPO, Wallace et al. 2023).

With L_b(p) the per-crystal denoising loss of the fine-tune step and both networks evaluated on the same noised input at the same time,
    d_b = L_b(agent) - L_b(prior),   pair p = (winner w, loser l):  loss_p = softplus(beta (d_w - d_l)) = -log sigmoid(-beta (d_w - d_l)),
    total = sum_p loss_p / (P accum_steps).
It needs no trajectory, no log-probability and no on-policy data: conditioned (fixed-formula) samples, replayed crystals, diversity-penalised
rewards, strided-chain samples and several sampling batches per loop are all usable, which policy.pg_step refuses.  One C call per timestep
(mi_dpo_micro_step: the fine-tune micro-step's noise, two forwards and backward, with the loss stage replaced), under finetune's epoch driver."""
import logging

import numpy as np
import torch

from . import _lib, streams
from .cspnet import _ptr, _stream
from .data import CrystalBatchData
from .dist import rank_world
from .finetune import _Config, _grad_buffer, _micro_step_operands, _run_epochs
from .optim import cfg_get, clip_options


def build_pairs(rewards, keys=None, margin=0.0, max_pairs=None, winners=None, seed=0):
    """(winner, loser) index pairs of `rewards` as an int64 array [P, 2]: every (w, l) with r_w - r_l > 0 and >= margin, with keys[w] ==
    keys[l] when `keys` is given and winners[w] when the boolean mask `winners` is given, in lexicographic (w, l) order.  More than
    `max_pairs` candidates: np.random.default_rng(seed).choice(count, max_pairs, replace=False) of them, in that order (sorted)."""
    r = np.asarray(rewards, dtype=np.float64).reshape(-1)
    n = len(r)
    diff = r[:, None] - r[None, :]
    ok = (diff > 0) & (diff >= float(margin))
    if keys is not None:
        assert len(keys) == n, "one key per reward"
        _, code = np.unique(np.asarray([repr(k) for k in keys]), return_inverse=True)
        ok &= code[:, None] == code[None, :]
    if winners is not None:
        w = np.asarray(winners, dtype=bool).reshape(-1)
        assert len(w) == n, "one mask entry per reward"
        ok &= w[:, None]
    pairs = np.argwhere(ok).astype(np.int64).reshape(-1, 2)   # (row-major: lexicographic in (w, l))
    if max_pairs is not None and len(pairs) > int(max_pairs):
        pairs = pairs[np.sort(np.random.default_rng(seed).choice(len(pairs), int(max_pairs), replace=False))]
    return pairs


def _dpo_micro_step(agent, prior, batch, time_idx, noise, beta, p_global, accum_steps, grad, stats, out_delta=None, out_margin=None,
                    call_id=None, aux_stream=None):
    """One timestep through mi_dpo_micro_step on the current stream; accumulates into `grad` (+=) and `stats` (device, 3 floats).  The
    agent's batch handle for `batch` must carry the pairs (CrystalBatch.set_pairs)."""
    head, (t,), sched, nz, aux = _micro_step_operands(agent, prior, batch, [time_idx], None if noise is None else [noise], aux_stream)
    if call_id is None:
        agent._noise_calls = getattr(agent, "_noise_calls", 0) + 1
        call_id = agent._noise_calls
    _lib.check(_lib.load().mi_dpo_micro_step(*head[:8], head[9], t, *(s[0] for s in sched), getattr(agent, "noise_seed", 0), call_id & 0xFFFFFFFF,
                                             _ptr(nz[0]), _ptr(nz[1]), _ptr(nz[2]), agent.cost_lattice, agent.cost_coord, agent.cost_type,
                                             beta, p_global, accum_steps, _ptr(grad), _ptr(stats), _ptr(out_delta), _ptr(out_margin), _stream(),
                                             aux), "mi_dpo_micro_step")


def dpo_step(agent, prior, data_list, pairs, cfg, device=None, noise_fn=None, log=logging.info):
    """cfg needs: lr, accum_steps, epochs, timesteps, dpo_beta (attribute or key access; there is no default for dpo_beta), and takes
    ft_step's optimiser options (max_grad_norm, skip_nonfinite_steps).  `pairs`: [P, 2] (winner, loser) indices into `data_list`
    (build_pairs).  Only the crystals that occur in a pair go into the batch (indices compacted, order kept).  Runs under finetune's epoch
    driver: a fresh fused Adam, an optimizer step wherever an accumulation window closes, one host read per epoch.  Returns the epochs'
    dicts: loss (mean over the timesteps of sum_p loss_p / P), pref_acc (the share of pair-timesteps with d_w < d_l), margin (the mean of
    d_l - d_w), and the optimiser's statistics when it clips or guards.  `noise_fn(epoch, t)` -> (rand_l, rand_x, rand_t) of the COMPACTED
    set injects noise (parity tests); default Philox, agent._noise_calls advancing once per timestep as in ft_step.
    Scope: one group, unstacked, one GPU, the DiffCSP module."""
    from .guidance import refuse_latent
    refuse_latent((agent, prior), "dpo_step")
    fields = _Config._fields[:4] + ("dpo_beta",)
    v = [cfg_get(cfg, k) for k in fields]
    if None in v:   # (before any device work)
        raise KeyError(f"dpo_step: the config has no {fields[v.index(None)]}")
    c = _Config(v[0], int(v[1]), int(v[2]), int(v[3]), None, clip_options(cfg))
    beta = float(v[4])
    if rank_world()[1] > 1:
        raise ValueError("dpo_step runs on one GPU: world_size > 1 is not supported (pairs cross shards)")
    if hasattr(agent, "collate"):
        raise ValueError("dpo_step needs the DiffCSP module: the MatterGen-shaped module has no fused micro-step to put the preference loss in")
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(pairs) == 0:
        raise ValueError("dpo_step: the pair list is empty")
    if pairs.min() < 0 or pairs.max() >= len(data_list):
        raise ValueError(f"dpo_step: a pair index lies outside the {len(data_list)} crystals")
    device = device or agent.device
    used, compact = np.unique(pairs.reshape(-1), return_inverse=True)
    compact = compact.reshape(-1, 2)
    n_pairs = len(compact)
    batch = CrystalBatchData([data_list[int(i)] for i in used])
    batch.reward = torch.zeros(len(used))   # (the micro-step's shared operands carry a reward column; this loss does not read it)
    batch = batch.to(device)
    agent.shard_offsets = prior.shard_offsets = (0, 0)
    aux = streams.concurrent_streams(2, device)[1]
    grad = _grad_buffer(agent.decoder.theta)
    ab = agent._batch_for(batch.num_atoms.cpu())
    torch.cuda.synchronize(device)   # (set_pairs copies with blocking copies: nothing of a cached handle may be in flight)
    ab.set_pairs(compact)

    def enqueue(epoch, t0, k, acc):
        _dpo_micro_step(agent, prior, batch, t0, None if noise_fn is None else noise_fn(epoch, t0), beta, n_pairs, c.accum_steps, grad, acc,
                        aux_stream=aux)
    try:
        return _run_epochs(agent, c, n_pairs, device, log, enqueue, keys=("loss", "pref_acc", "margin"), where="dpo_step")
    finally:
        torch.cuda.synchronize(device)
        ab.set_pairs(None)

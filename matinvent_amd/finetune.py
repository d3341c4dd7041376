"""The reward-weighted fine-tune step (MatInvent.ft_step, pipeline/mat_invent.py:125-189).

    loss = mean_b( r_b * L_dsm(b, t) + sigma * (1.1 - r_b) * ||pred_agent - pred_prior||^2 ) / accum_steps

accumulated over `accum_steps` timesteps per optimizer step, `epochs` passes over the `timesteps`
grid, a fresh Adam per call.  Differences from the reference, none of which change the update:
  * the three `.item()` host syncs per timestep (:168-170) become device-side accumulators read once
    per epoch;
  * data parallel: every rank holds a contiguous shard of the fine-tune set, scales its local sum by
    1/(B_global * accum_steps) (the reference's `.mean()` over the whole batch, :163) and one flat
    all-reduce of the gradient precedes each optimizer step; every rank applies the same fused Adam.
"""
import ctypes as C
import logging
import sys
from collections import namedtuple

import torch

from . import _lib, streams
from .cspnet import _ptr, _stream
from .data import CrystalBatchData, CrystalDataset
from .dist import allreduce_flat_, rank_world, shard_range
from .optim import FusedAdam, cfg_get, clip_options, epoch_grad_stats, window_closes


def _sched_host(agent):
    """Host copies of the noise schedules (made once per module): indexing the device tensors costs a device sync per scalar and
    timestep, which the launch-bound small-set regime cannot afford."""
    bufs = (agent.beta_scheduler.alphas_cumprod, agent.sigma_scheduler.sigmas, agent.sigma_scheduler.sigmas_norm)
    key = tuple((b.data_ptr(), b._version) for b in bufs)  # a checkpoint load after the first ft_step changes the buffers
    h = agent.__dict__.get("_mi_sched_host")
    if h is None or h[0] != key:
        ac = bufs[0].detach().cpu()
        h = agent.__dict__["_mi_sched_host"] = (key, (torch.sqrt(ac).tolist(), torch.sqrt(1.0 - ac).tolist(),
                                                      bufs[1].detach().cpu().tolist(), bufs[2].detach().cpu().tolist()))
    return h[1]


def _host_atoms(batch):
    """The batch's atom counts on the host, copied once per batch: no device synchronisation per timestep."""
    return batch.__dict__.setdefault("_mi_na", batch.num_atoms.cpu())


def _micro_step_operands(agent, prior, batch, time_idxs, noises, aux_stream):
    """What mi_ft_micro_step and mi_ft_micro_steps_stacked share, for the k = len(time_idxs) timesteps of one call.  Returns the leading
    arguments of both entries (both networks with their batch handles over k replicas of the set, the packed weights of both brought up to
    date; the set's arrays on the device, repeated k times and cached on the batch per k, three entries at most; the time embedding), the k
    chain times with their four schedule values (host lists), the injected noise (`noises`: k tuples, the replicas' rows one after the
    other; or None) and the auxiliary stream's handle."""
    dev = agent.device
    k = len(time_idxs)
    T = agent.beta_scheduler.timesteps
    ts = [T - int(i) for i in time_idxs]
    na = _host_atoms(batch) if k == 1 else _host_atoms(batch).repeat(k)
    ab, pb = agent._batch_for(na), prior._batch_for(na)
    agent.decoder.sync()
    prior.decoder.sync()
    sched = [[s[t] for t in ts] for s in _sched_host(agent)]   # sqrt(alpha_bar), sqrt(1 - alpha_bar), sigma, sigma_norm
    cache = batch.__dict__.setdefault("_mi_dev", {})
    if k not in cache:
        f = lambda x: x.to(dev, torch.float32).contiguous()
        rep = (lambda x: x) if k == 1 else (lambda x: x.repeat(k, *([1] * (x.dim() - 1))).contiguous())
        cache[k] = dict(lengths=rep(f(batch.lengths)), angles=rep(f(batch.angles)), frac=rep(f(batch.frac_coords)),
                        types=rep(batch.atom_types.to(dev, torch.int32).contiguous()), reward=rep(f(batch.reward)))
        while len(cache) > 3:
            cache.pop(next(iter(cache)))
    c = cache[k]
    nz = (None, None, None)
    if noises is not None:  # injected noise (parity tests)
        cols = ([n[j].to(dev, torch.float32) for n in noises] for j in range(3))
        nz = tuple((col[0] if k == 1 else torch.cat(col)).contiguous() for col in cols)
    head = (agent.decoder._h, ab._h, prior.decoder._h, pb._h, _ptr(c["lengths"]), _ptr(c["angles"]), _ptr(c["frac"]), _ptr(c["types"]),
            _ptr(c["reward"]), _ptr(agent.time_embedding.freqs))
    return head, ts, sched, nz, C.c_void_p(aux_stream.cuda_stream) if aux_stream is not None else None


def _fused_micro_step(agent, prior, batch, time_idx, noise, sigma, n_global, accum_steps, grad, stats, call_id=None, aux_stream=None):
    """One timestep through mi_ft_micro_step on the current stream; accumulates into `grad` (+=) and `stats` (device, 3
    floats).  `call_id` = the noise-stream call counter (one value per timestep, shared by every crystal group)."""
    head, (t,), sched, nz, aux = _micro_step_operands(agent, prior, batch, [time_idx], None if noise is None else [noise], aux_stream)
    if call_id is None:
        agent._noise_calls = getattr(agent, "_noise_calls", 0) + 1
        call_id = agent._noise_calls
    _lib.check(_lib.load().mi_ft_micro_step(*head, t, *(s[0] for s in sched), getattr(agent, "noise_seed", 0), call_id & 0xFFFFFFFF,
                                            _ptr(nz[0]), _ptr(nz[1]), _ptr(nz[2]), agent.cost_lattice, agent.cost_coord, agent.cost_type,
                                            sigma, n_global, accum_steps, _ptr(grad), _ptr(stats), None, None, _stream(), aux),
               "mi_ft_micro_step")


def _stacked_micro_steps(agent, prior, batch, time_idxs, noises, sigma, n_global, accum_steps, grad, stats, aux_stream=None):
    """`len(time_idxs)` consecutive timesteps of one accumulation window as ONE micro-step over a batch holding that many replicas
    of the fine-tune set (mi_ft_micro_steps_stacked): the same gradient and statistics as calling _fused_micro_step once per
    timestep, with a fraction of the kernel launches -- a single timestep of a small set is bound by the host's launch rate."""
    k = len(time_idxs)
    head, ts, sched, nz, aux = _micro_step_operands(agent, prior, batch, time_idxs, noises, aux_stream)
    call0 = getattr(agent, "_noise_calls", 0) + 1  # replica j uses the call id of its own timestep
    agent._noise_calls = call0 + k - 1
    arr = lambda ctype, vals: (ctype * k)(*vals)
    _lib.check(_lib.load().mi_ft_micro_steps_stacked(*head, k, arr(C.c_int, ts), *(arr(C.c_float, s) for s in sched),
                                                     getattr(agent, "noise_seed", 0), call0 & 0xFFFFFFFF, _ptr(nz[0]), _ptr(nz[1]),
                                                     _ptr(nz[2]), agent.cost_lattice, agent.cost_coord, agent.cost_type, sigma, n_global,
                                                     accum_steps, _ptr(grad), _ptr(stats), _stream(), aux), "mi_ft_micro_steps_stacked")


MAX_STACK = 16  # MI_MAX_STACK of the C ABI
FT_PRIOR_AUX = False  # grouped path: the frozen prior's forward of every group on an auxiliary stream (measured: see DESIGN 20)
WGRAD_WINDOW = 16  # micro-steps whose node-level weight gradients are contracted together (mi_batch_set_wgrad_window); 0 = off


def auto_groups(e_total: int) -> int:
    """Concurrent crystal groups ft_step picks for a local set with `e_total` directed edges (measured at 256 x 20 atoms, round 3:
    16.1k / 16.7k / 17.3k / 13.9k / 11.7k crystal-timesteps/s with 2 / 3 / 4 / 6 / 8 groups)."""
    # (round 6, after the fused backward chain and the contractions' share of the chip: 128 crystals x 20 atoms on 1 / 2 / 3 groups 16.3k / 17.0k / 17.6k,
    #  64 crystals 12.65k / 12.46k / 12.1k, 256 crystals on 3 / 4 / 5 groups 21.3k / 21.7k / 17.0k: profiles/r6_strong_shapes.json)
    return 4 if e_total >= 90000 else 3 if e_total >= 40000 else 1


def _stack_plan(e_one, accum_steps, timesteps, stack):
    """Chunk sizes of the timestep loop: every chunk lies inside one accumulation window.  stack=None: as many timesteps per
    chunk as bring the stacked batch to ~32k edges (beyond that a micro-step is no longer launch-bound), evenly sized."""
    if stack is None:
        stack = max(1, min(MAX_STACK, 32768 // max(1, e_one)))
    stack = max(1, min(int(stack), MAX_STACK))
    plan, t = [], 0
    while t < timesteps:
        w = min(accum_steps - t % accum_steps, timesteps - t)  # timesteps left in this window
        n = -(-w // stack)                                     # chunks for them, sized evenly
        sizes = [w // n + (1 if j < w % n else 0) for j in range(n)]
        plan += sizes
        t += w
    return plan


_Config = namedtuple("_Config", "lr accum_steps epochs timesteps sigma opt")   # a fine-tune config as ft_step reads it; opt: FusedAdam's options


def _grad_buffer(theta):
    """theta.grad, allocated (zero) where there is none yet: the fused micro-steps accumulate into it, and a rank without data reduces it."""
    if theta.grad is None:
        theta.grad = torch.zeros_like(theta)
    return theta.grad


def _run_epochs(agent, c, n_global, device, log, enqueue, plan=None, start=None, collect=None, before_step=None, after_step=None,
                keys=None, where="ft_step"):
    """What every route of ft_step shares: a fresh fused Adam, `c.epochs` passes over the timesteps, an optimizer step -- all-reduce of the
    flat gradient, Adam, zero -- wherever an accumulation window closes, one reduction and one host read at the end of an epoch, its dict
    and log line.  A route plugs in what is its own:
      enqueue(epoch, t0, k, acc)   enqueues the timesteps t0 .. t0 + k - 1 (k = the entries of `plan`, each inside one window; default:
                                   one timestep at a time), accumulating into theta.grad and `acc`;
      start()                      what an epoch starts with; returns its loss / loss_diff / loss_kl accumulators (default: three device floats);
      collect(acc)                 the three sums of the epoch from what start() returned (default: `acc` itself);
      before_step(), after_step()  what surrounds an optimizer step (default: nothing);
      keys, where                  the names of its three accumulators in the epoch dicts (default: ft_step's loss / loss_diff / loss_kl) and
                                   its name in an error message.
    Every rank must come here with the same `c.opt`, the rank without data included: one that clips differently diverges from its peers."""
    theta = agent.decoder.theta
    rank = rank_world()[0]
    optimizer = FusedAdam([theta], lr=c.lr, **c.opt)  # fresh every call (:136); the norm it clips is the all-reduced one
    plan = [1] * c.timesteps if plan is None else plan
    stats = []
    for epoch in range(c.epochs):
        agent.train()
        if theta.grad is not None:
            optimizer.zero_grad(set_to_none=False)
        acc = torch.zeros(3, device=device) if start is None else start()  # loss, loss_diff, loss_kl accumulators (device side)
        t = 0
        for k in plan:
            enqueue(epoch, t, k, acc)
            t += k
            if window_closes(t, c.accum_steps, c.timesteps):                      # :165-167, :176-177
                if before_step is not None:
                    before_step()
                allreduce_flat_(theta.grad)
                optimizer.step()
                optimizer.zero_grad(set_to_none=False)
                if after_step is not None:
                    after_step()
        d = _epoch_stats(_epoch_reduce(acc if collect is None else collect(acc), where, optimizer), c.timesteps, n_global,
                         *(() if keys is None else (keys,)))
        stats.append(d)
        if rank == 0:
            log(f"Epoch {epoch}: " + ", ".join(f"{k}: {v:.4f}" for k, v in d.items()))
    return stats


def ft_step(agent, prior, data_list, rewards, cfg, device=None, noise_fn=None, log=logging.info, fused=True, groups=None, stack=None):
    """cfg needs: lr, accum_steps, epochs, timesteps, sigma (attribute or key access).
    `noise_fn(epoch, t)` -> (rand_l, rand_x, rand_t) injects noise (parity tests); default Philox.
    fused=True (default) enqueues each timestep through mi_ft_micro_step (noise, both forwards, the fused
    loss / penalty / gradient-seed kernel and the backward in one C call, no autograd graph); fused=False
    drives the same arithmetic through the reference's module surface (add_noise / calc_sample_loss /
    calc_kl_reg + autograd), which is what the parity tests compare it with.  A module with `collate` (the MatterGen-shaped one)
    always takes that loop (_surface_timestep), over chunks of its set.  Every route runs under one epoch driver (_run_epochs).
    `groups` (fused path): the local fine-tune set is cut into that many contiguous crystal groups whose micro-steps are
    enqueued on separate HIP streams and run concurrently, each accumulating into its own gradient buffer (summed before
    the optimizer step) -- the same arithmetic as data-parallel ranks, inside one GPU: one group's node-level and
    reduction kernels overlap the other's large GEMMs.  None = automatic (2-3 for large sets; measured at 256 x 20 atoms:
    16.1k / 16.7k / 17.3k / 13.9k crystal-timesteps/s with 2 / 3 / 4 / 6 groups, round 3).
    `stack` (fused path, single group): up to that many consecutive timesteps of an accumulation window run as ONE stacked
    micro-step (the weights only change at the optimizer step, so they are independent; same noise, same gradient up to fp32
    summation order).  None = automatic (small sets, which are bound by the host's launch rate); 1 = off.
    cfg.max_grad_norm (a number > 0) / cfg.skip_nonfinite_steps (bool), both optional: every optimizer step clips the gradient to that
    global norm / leaves out a step whose gradient holds inf or NaN, on the device inside FusedAdam.step (optim.py); the epoch
    dicts then also carry grad_norm, grad_norm_max, clipped_steps, skipped_steps.  The norm is taken after the all-reduce of the gradient
    (and after the groups' gradients are summed), so every rank computes the same coefficient and takes the same decision."""
    from .guidance import refuse_latent
    refuse_latent((agent, prior), "ft_step")
    v = [cfg_get(cfg, k) for k in _Config._fields[:5]]
    if None in v:   # (before any device work)
        raise KeyError(f"ft_step: the config has no {_Config._fields[v.index(None)]}")
    c = _Config(v[0], int(v[1]), int(v[2]), int(v[3]), v[4], clip_options(cfg))   # opt: read once, the same on every route below
    device = device or agent.device
    rank, world = rank_world()
    n_global = len(data_list)
    lo, hi = shard_range(n_global, rank, world)
    surface = hasattr(agent, "collate")   # MatterGen-shaped module: its own records / collate, always over the module surface
    dataset = None if surface else CrystalDataset(data_list, rewards)
    theta = agent.decoder.theta
    if hi == lo:
        # fewer crystals than ranks (the fine-tune set is top-k + replay and shrinks when the validity filter keeps few samples):
        # this rank has nothing to differentiate, but must take part in every all-reduce and apply every optimizer step
        _grad_buffer(theta)

        def start():
            # the Philox call id advances once per timestep on the ranks that hold data: keep this rank's counter in step, so that the noise of
            # later ft_steps does not depend on which ranks had empty shards before (world-size invariance of the global-id noise)
            agent._noise_calls = getattr(agent, "_noise_calls", 0) + c.timesteps
            return torch.zeros(3, device=theta.device)
        return _run_epochs(agent, c, n_global, device, log, lambda *_: None, start=start)
    if surface:
        return _run_epochs(agent, c, n_global, device, log, _surface_timestep(
            agent, prior, _surface_chunks(agent, data_list, rewards, lo, hi, device, noise_fn), c, n_global, noise_fn,
            _surface_aux_stream(device)))
    # one batch holding the whole (local shard of the) fine-tune set (:129-133); order is irrelevant to the update
    batch = CrystalBatchData([dataset[i] for i in range(lo, hi)]).to(device)
    node_lo = sum(d.num_atoms for d in dataset.data_list[:lo])
    agent.shard_offsets = prior.shard_offsets = (node_lo, lo)
    if not fused:   # the parity path: the prior through calc_sample_loss on the current stream, as the reference evaluates it
        return _run_epochs(agent, c, n_global, device, log, _surface_timestep(agent, prior, [(batch, (node_lo, lo))], c, n_global, noise_fn, None))
    e_local = sum(d.num_atoms ** 2 for d in dataset.data_list[lo:hi])
    groups = max(1, min(int(auto_groups(e_local) if groups is None else groups), hi - lo))
    if groups > 1:
        return _ft_step_grouped(agent, prior, dataset, lo, hi, node_lo, n_global, groups, c, device, noise_fn, log)
    aux = streams.concurrent_streams(2, device)[1]   # a single (small) group: fork the frozen prior's forward onto a second, really concurrent stream
    grad = _grad_buffer(theta)

    def enqueue(epoch, t0, k, acc):
        noises = None if noise_fn is None else [noise_fn(epoch, i) for i in range(t0, t0 + k)]
        if k == 1:   # (the stacked entry with one replica sums in another order: the single entry keeps its bits)
            _fused_micro_step(agent, prior, batch, t0, None if noises is None else noises[0], c.sigma, n_global, c.accum_steps, grad, acc,
                              aux_stream=aux)
        else:
            _stacked_micro_steps(agent, prior, batch, list(range(t0, t0 + k)), noises, c.sigma, n_global, c.accum_steps, grad, acc,
                                 aux_stream=aux)
    return _run_epochs(agent, c, n_global, device, log, enqueue, plan=_stack_plan(e_local, c.accum_steps, c.timesteps, stack))


def _epoch_stats(a, timesteps, n_global, keys=("loss", "loss_diff", "loss_kl")):
    """An epoch's dict from _epoch_reduce's list: the three losses under the route's `keys` (the first a mean over the timesteps, the other
    two also over n_global); behind them, when the optimizer clips or guards, its statistics."""
    d = {keys[0]: a[0] / timesteps, keys[1]: a[1] / timesteps / n_global, keys[2]: a[2] / timesteps / n_global}
    if len(a) > 3:
        d.update(epoch_grad_stats(a[3:]))
    return d


def _epoch_reduce(acc, where, optimizer=None):
    """End of an epoch on every rank: sum the loss accumulators over the ranks and, in the same collective, the ranks' saturation counts
    of the two-plane fp16 format -- a rank-local check would raise on one rank while its peers go on to the next epoch's all-reduces
    (a hang instead of an error).  Returns the accumulators as a list; raises FloatingPointError on EVERY rank when any rank saturated.
    An `optimizer` that clips or guards (FusedAdam.guarded): its statistics of the epoch ride in the same transfer and follow the
    accumulators in the list (optim.GRAD_STATS order); they are the same on every rank, so rank 0's are the ones summed."""
    n_local = _lib.saturation_events(reset=True)   # (synchronises the device: the epoch's kernels have finished)
    if optimizer is not None and optimizer.guarded:
        g = optimizer.grad_stats(reset=True).to(torch.float32)
        acc = torch.cat([acc.to(torch.float32), g if rank_world()[0] == 0 else torch.zeros_like(g)])
    buf = torch.cat([acc.to(torch.float32), torch.tensor([float(min(n_local, 1 << 24))], device=acc.device)])
    allreduce_flat_(buf)
    a = buf.tolist()  # the only host read of the epoch
    if a[-1] > 0:
        raise FloatingPointError(
            f"{where}: {int(a[-1])} operand conversions (summed over the ranks; {n_local} on this one) saturated the two-plane fp16 format "
            "(values beyond 65504 / scale, or NaN / inf upstream): the results are outside the stated fp32-class tolerance.  Rebuild with "
            "MI_EXTRA_FLAGS=-DMI_PLANES_FP16=0 (three bf16 planes, no range limit) or use --path f32-gemm")
    return a[:-1]


PRIOR_ON_AUX_STREAM = True   # module-surface loop of a MatterGen-shaped module: the frozen prior's forward concurrently with the agent's


def _surface_chunks(agent, data_list, rewards, lo, hi, device, noise_fn):
    """The local shard of a MatterGen-shaped module's set as [(batch, shard offsets)] chunks of at most FT_CHUNK_ATOMS atoms: the training
    forward keeps every activation for the backward, and the whole benchmark set (256 crystals x 20 atoms: 171 GB of activations + as much
    again for their gradients) does not fit one GPU.  The update is linear in the per-crystal losses (sum / (n_global * accum_steps)), the
    noise is indexed by global atom / crystal ids, so chunking changes nothing but the summation order of the gradient.  Injected noise
    (parity tests) spans the shard: one chunk."""
    from .mattergen import FT_CHUNK_ATOMS
    bounds, c0, atoms = [], lo, 0
    for i in range(lo, hi):
        n_i = int(data_list[i].num_atoms)
        if i > c0 and atoms + n_i > FT_CHUNK_ATOMS and noise_fn is None:
            bounds.append((c0, i))
            c0, atoms = i, 0
        atoms += n_i
    bounds.append((c0, hi))
    chunks = []
    for (a_, b_) in bounds:
        cb = agent.collate(data_list[a_:b_], None if rewards is None else list(rewards[a_:b_])).to(device)
        chunks.append((cb, (sum(d.num_atoms for d in data_list[:a_]), a_)))
    return chunks


def _surface_aux_stream(device):
    """The stream the frozen prior's forward of the module-surface loop runs on (None: serial): one of a concurrent pair that is not the current one."""
    if not (PRIOR_ON_AUX_STREAM and torch.device(device).type == "cuda"):
        return None
    aux = streams.concurrent_streams(2, device)[1]
    return streams.concurrent_streams(2, device)[0] if aux == torch.cuda.current_stream() else aux


def _surface_timestep(agent, prior, chunks, c, n_global, noise_fn, aux):
    """_run_epochs' `enqueue` over the module surface: pipeline/mat_invent.py:150-164 literally (add_noise / calc_sample_loss / calc_kl_reg;
    the network is one differentiable op with a hand-written backward) for every (batch, shard offsets) of `chunks`, with device-side loss
    accumulators and the data-parallel scaling of ft_step.  `aux`: a stream for the frozen prior's forward (a prior with `predict`)."""
    def enqueue(epoch, t, k, acc):
        noise = None if noise_fn is None else noise_fn(epoch, t)
        calls = getattr(agent, "_noise_calls", 0)
        for batch, offs in chunks:
            agent.shard_offsets = prior.shard_offsets = offs
            agent._noise_calls = calls                                            # (every chunk of a timestep draws from the same Philox step)
            noised = agent.add_noise(batch, t, noise=noise)                       # :152
            if aux is not None and hasattr(prior, "predict"):
                # the frozen prior's forward on a second stream, under the agent's (separate network and batch handle).  Only the two
                # NETWORK evaluations overlap -- kernels of this library, built without packed-fp32 instructions; the loss
                # arithmetic is torch's own elementwise kernels, which are not, and runs after the join with nothing beside it.  (The
                # prior's sample loss, line :154 of the reference, is computed there and never used: only its prediction is needed.)
                aux.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(aux), torch.no_grad():
                    prior_pred = prior.predict(noised)                            # :154
                agent_out = agent.predict(noised)
                torch.cuda.current_stream().wait_stream(aux)
                for v in (prior_pred.values() if isinstance(prior_pred, dict) else prior_pred):
                    if torch.is_tensor(v) and v.is_cuda:
                        v.record_stream(torch.cuda.current_stream())
                sample_loss, agent_pred = agent.calc_sample_loss(noised, pred=agent_out)   # :153
            else:
                sample_loss, agent_pred = agent.calc_sample_loss(noised)          # :153
                with torch.no_grad():
                    _, prior_pred = prior.calc_sample_loss(noised)                # :154 (frozen prior)
            loss_diff = batch.reward * sample_loss                                # :158
            loss_kl = agent.calc_kl_reg(agent_pred, prior_pred, batch) * (1.1 - batch.reward)   # :160-161
            loss = (loss_diff + loss_kl * c.sigma).sum() / (n_global * c.accum_steps)  # == .mean() / accum_steps (:163)
            loss.backward()
            with torch.no_grad():
                acc += torch.stack([loss.detach() * c.accum_steps, loss_diff.detach().sum(), loss_kl.detach().sum()])
    return enqueue


def _ft_step_grouped(agent, prior, dataset, lo, hi, node_lo, n_global, groups, c, device, noise_fn, log):
    """ft_step's fused path with the local set cut into `groups` crystal groups on concurrent streams (see ft_step)."""
    theta = agent.decoder.theta
    cuts = [lo + (hi - lo) * k // groups for k in range(groups + 1)]
    offs = [(node_lo, lo)]   # (first atom, first crystal) of every group, global ids; behind them the end of the last group
    for k in range(groups):
        offs.append((offs[-1][0] + sum(d.num_atoms for d in dataset.data_list[cuts[k]:cuts[k + 1]]), cuts[k + 1]))
    batches = [CrystalBatchData([dataset[i] for i in range(cuts[k], cuts[k + 1])]).to(device) for k in range(groups)]
    # injected noise (rand_l [B,3,3], rand_x [N,3], rand_t [N,100]) of the local set -> every group's crystal rows and atom rows
    rows = [(slice(a[1] - lo, b[1] - lo), slice(a[0] - node_lo, b[0] - node_lo)) for a, b in zip(offs, offs[1:])]
    main = torch.cuda.current_stream()
    gstreams = streams.concurrent_streams(groups, device)
    # FT_PRIOR_AUX (experiment, MI_FT_PRIOR_AUX=1): every group forks its frozen prior's forward onto a stream of its own, as the single-group path does
    aux_streams = streams.concurrent_streams(2 * groups, device)[groups:] if FT_PRIOR_AUX else [None] * groups
    grads = [_grad_buffer(theta)] + [torch.zeros_like(theta) for _ in range(groups - 1)]
    # The weights only change at the optimizer step, so the node-level linears' weight gradients of a run of micro-steps are ONE
    # contraction over all their rows instead of one short contraction (1.7k rows per group at 256 x 20 atoms) per micro-step: the
    # agent's batch handles keep the operand rows of up to WGRAD_WINDOW micro-steps (see include/matinvent_hip.h).
    # `cap`: the window a LATER call on these handles may ask for (its timesteps are not known here) -- the buffers are sized for it once, so that a short first
    # call (a warm-up of three timesteps) is not followed by a reallocation -- sixteen hipFree / hipMalloc pairs per group, each a device synchronisation -- at the
    # start of the next one (measured: a 20-timestep call behind a 3-timestep warm-up ran at 13.1 k instead of 19-21 k crystal-timesteps/s)
    cap = min(c.accum_steps, WGRAD_WINDOW) if groups <= 8 else 0   # (_batch_for caches eight handles per module)
    dec = agent.decoder
    nmax_ = max(b[0] - a[0] for a, b in zip(offs, offs[1:]))
    slot_bytes = (7 * dec.hidden_dim * dec.num_layers + 4 * dec.hidden_dim + 203) * nmax_ * 4   # operand rows of one micro-step: node-level linears + heads / embedding
    # at most 8 GB of kept rows per group AND 24 GB over all groups (the windows of the groups are live together)
    cap = max(0, min(cap, (8 << 30) // max(1, slot_bytes), (24 << 30) // max(1, slot_bytes * groups)))
    window = min(cap, c.timesteps)
    handles = []
    for k in range(groups):
        agent.shard_offsets = offs[k]
        handles.append(agent._batch_for(_host_atoms(batches[k])))
    try:
        for ab in handles:
            if cap > window > 1:
                ab.set_wgrad_window(agent.decoder, cap)   # (reserves the buffers; the line below only lowers the slot count)
            ab.set_wgrad_window(agent.decoder, window if window > 1 else 0)
    except _lib.MIError as e:   # the window is an optimisation: out of memory for it -> the immediate form, not a failed fine-tune step
        if e.code != _lib.MI_ENOMEM:
            raise
        window = 0
        for ab in handles:
            ab.set_wgrad_window(agent.decoder, 0)

    def flush_wgrads():
        for k in range(groups):
            with torch.cuda.stream(gstreams[k]):
                handles[k].wgrad_flush(agent.decoder, grads[k])

    def release():   # the group streams go on behind what the main stream holds now
        ready = main.record_event()
        for st in gstreams:
            st.wait_event(ready)

    def join():      # the main stream goes on behind what every group stream holds now
        for st in gstreams:
            main.wait_event(st.record_event())

    def start():
        accs = [torch.zeros(3, device=device) for _ in range(groups)]
        agent.decoder.sync()
        prior.decoder.sync()
        release()
        return accs

    def enqueue(epoch, t, _, accs):   # one micro-step per group, all with the timestep's one noise call id
        noise = None if noise_fn is None else noise_fn(epoch, t)
        agent._noise_calls = getattr(agent, "_noise_calls", 0) + 1
        for k in range(groups):
            nz = None if noise is None else (noise[0][rows[k][0]], noise[1][rows[k][1]], noise[2][rows[k][1]])
            agent.shard_offsets = prior.shard_offsets = offs[k]
            with torch.cuda.stream(gstreams[k]):
                _fused_micro_step(agent, prior, batches[k], t, nz, c.sigma, n_global, c.accum_steps, grads[k], accs[k],
                                  call_id=agent._noise_calls, aux_stream=aux_streams[k])

    def before_step():   # the optimizer consumes (and clips) the SUM of the groups' gradients
        flush_wgrads()
        join()
        for g in grads[1:]:
            theta.grad.add_(g)
            g.zero_()

    def after_step():    # repack the updated weights once, on the main stream, before any group reads them
        agent.decoder.sync()
        release()

    def collect(accs):
        join()
        return torch.stack(accs).sum(0)

    was_groups = _lib.load().mi_set_concurrent_groups(groups)   # (each group's weight-gradient contractions take their share of the chip, not all of it)
    try:
        stats = _run_epochs(agent, c, n_global, device, log, enqueue, start=start, collect=collect, before_step=before_step, after_step=after_step)
        agent.shard_offsets = prior.shard_offsets = (node_lo, lo)
        return stats
    finally:
        _lib.load().mi_set_concurrent_groups(was_groups)
        failing = sys.exc_info()[0] is not None
        try:   # (nothing pending unless an exception cut a window short -- and then its own error must not replace that exception)
            flush_wgrads()
            for ab in handles:
                ab.set_wgrad_window(agent.decoder, 0)
        except Exception:
            if not failing:
                raise

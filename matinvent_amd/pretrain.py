"""Supervised denoising training of a DiffCSP prior on a crystal dataset (DiffCSPModule.training_step, models/diffcsp/diffusion.py:457-486,
driven over epochs of shuffled mini-batches).

    loss = cost_lattice mse(pred_l, rand_l) + cost_coord mse(pred_x, tar_x) + cost_type mse(pred_t, rand_t)

with one uniformly drawn time per crystal and torch's F.mse_loss over ALL elements of the mini-batch (every atom weighs the same).  One
network, no reward, no anchor: each micro-step is mi_pretrain_micro_step (include/matinvent_hip_pretrain.h) -- the time gather, the
noising, the taped forward, the loss with its gradient seeds and statistics, the backward -- enqueued with no host synchronisation.

Everything random is a function of (seed, epoch, step): the mini-batches (batch_plan), the times (draw_times) and the Philox noise (one
call id per micro-step, indexed by the crystal's and the atom's position in the mini-batch, so data-parallel shards draw what the whole
mini-batch draws).  A mini-batch's batch handle is created for its atom counts and released after its micro-step: device memory does
not grow with the number of distinct mini-batches, and the module's handle cache (sampling, ft_step) is left alone.
"""
import contextlib
import ctypes as C
import logging
import os
import tempfile

import numpy as np
import torch

from . import _lib
from .cspnet import _ptr, _stream
from .data import CrystalBatchData
from .dist import allreduce_flat_, rank_world, shard_range
from .optim import FusedAdam, cfg_get, clip_options, ema_decay_at, epoch_grad_stats, parse_ema, window_closes
from .pool import HandlePool, parse_handle_pool

STATS = ("loss", "loss_lattice", "loss_coord", "loss_type")   # mi_pretrain_micro_step's stats[0..3]
_PLAN_TAG, _TIME_TAG = 0x706C616E, 0x74696D65                 # (the two generators never share a key)
EVAL_CALL = 0                                                 # the Philox call id of `evaluate` (training counts from 1)


def batch_plan(n, batch_size, epoch, seed, shuffle=True):
    """The index lists of one epoch's mini-batches over a set of `n`: a permutation of range(n) from a numpy Generator keyed by
    (seed, epoch) -- or range(n) itself -- cut into runs of `batch_size`, the last one partial.  A function of its arguments only."""
    n, batch_size = int(n), int(batch_size)
    if batch_size < 1:
        raise ValueError(f"batch_size = {batch_size}: must be >= 1")
    order = np.random.default_rng([_PLAN_TAG, int(seed), int(epoch)]).permutation(n) if shuffle else np.arange(n)
    return [order[s:s + batch_size].tolist() for s in range(0, n, batch_size)]


def draw_times(B, T, epoch, step, seed):
    """[B] int32 times, uniform in 1..T like BetaScheduler.uniform_sample_t (scheduler.py:90-92), from a numpy Generator keyed by
    (seed, epoch, step)."""
    return np.random.default_rng([_TIME_TAG, int(seed), int(epoch), int(step)]).integers(1, int(T) + 1, size=int(B)).astype(np.int32)


def _refuse(model, where):
    """The modules this training is not for (ValueError, before any device work)."""
    if getattr(model, "base", None) is not None:
        raise ValueError(f"{where}: a respaced view is for sampling; train its .base, the module of the trained grid")
    if hasattr(model, "collate"):
        raise ValueError(f"{where}: the MatterGen-shaped module has no supervised training here (DiffCSP only)")


def schedule_table(model):
    """[T + 1][4] float32 on the device: sqrt(alpha_bar_t), sqrt(1 - alpha_bar_t), sigma_t, sigmas_norm_t -- add_noise's four scalars of
    every time, cached on the module until a scheduler buffer changes (checkpoint load)."""
    bufs = (model.beta_scheduler.alphas_cumprod, model.sigma_scheduler.sigmas, model.sigma_scheduler.sigmas_norm)
    key = tuple((b.data_ptr(), b._version) for b in bufs) + (str(model.device),)
    h = model.__dict__.get("_mi_sched_table")
    if h is None or h[0] != key:
        ac = bufs[0]
        tab = torch.stack([torch.sqrt(ac), torch.sqrt(1.0 - ac), bufs[1], bufs[2]], dim=1).to(model.device, torch.float32).contiguous()
        h = model.__dict__["_mi_sched_table"] = (key, tab)
    return h[1]


def _counts(batch):
    na = batch.num_atoms
    return [int(v) for v in (na.tolist() if torch.is_tensor(na) else na)]


def train_step(model, batch, times, noise=None, grad=None, stats=None, b_global=None, n_global=None, accum_steps=1, seed=0, call_id=None,
               offsets=(0, 0), forward_only=False, out_parts=None, pool=None, y=None, p_uncond=0.0):
    """One fused micro-step on the current stream: `batch` (num_atoms, lengths, angles, frac_coords, atom_types; a CrystalBatchData) at
    the per-crystal `times` ([B] ints in 1..T).  Accumulates (+=) into `grad` (default: theta.grad, allocated when absent) and `stats`
    (4 device floats in STATS order; returned).  noise = (rand_l, rand_x, rand_t) injects the draws; otherwise Philox draws 7-9 at
    `call_id` (default: the module's running counter, advanced) with the handle's `offsets` = (first atom, first crystal) of this shard
    in the mini-batch.  b_global / n_global: the crystal / atom counts the loss is normalised by (default: the batch's own).
    forward_only=True: no tape, no backward, `grad` untouched (the validation loss).  The batch handle lives for this call only.
    pool: a pool.HandlePool of the current stream -- the handle's memory comes from it and goes back to it, and this call waits for
    nothing; None: the handle allocates and frees its own memory, which waits for the micro-step.
    A property-conditioned module runs mi_pretrain_micro_step_cond: y = the crystals' raw property values [B][P] (NaN: missing;
    None: every crystal under the null condition), p_uncond = the probability with which the device drops a crystal's condition (draw id 28
    at `call_id`, indexed through offsets[1]: guidance.drop_mask is the same draw on the host)."""
    _refuse(model, "train_step")
    cond = getattr(model, "condition", None)
    if cond is None and (y is not None or float(p_uncond) != 0.0):
        raise ValueError("train_step: y / p_uncond need a property-conditioned module (latent_dim > 0)")
    if not 0.0 <= float(p_uncond) <= 1.0:
        raise ValueError(f"train_step: p_uncond = {p_uncond} lies outside [0, 1]")
    lib = _lib.load()
    dev = model.device
    na = _counts(batch)
    B, N = len(na), sum(na)
    T = model.beta_scheduler.timesteps
    th = np.ascontiguousarray(np.asarray(times.cpu() if torch.is_tensor(times) else times), dtype=np.int32).reshape(-1)
    if th.shape[0] != B:
        raise ValueError(f"train_step: {th.shape[0]} times for {B} crystals")
    if B and (int(th.min()) < 1 or int(th.max()) > T):
        raise ValueError(f"train_step: times must lie in 1..{T} (got {int(th.min())}..{int(th.max())})")
    theta = model.decoder.theta
    if stats is None:
        stats = torch.zeros(4, device=dev)
    if not forward_only and grad is None:
        if theta.grad is None:
            theta.grad = torch.zeros_like(theta)
        grad = theta.grad
    if call_id is None:
        model._noise_calls = getattr(model, "_noise_calls", 0) + 1
        call_id = model._noise_calls
    if B == 0:
        return stats
    f = lambda x: x.to(dev, torch.float32).contiguous()
    lengths, angles, frac0 = f(batch.lengths), f(batch.angles), f(batch.frac_coords)
    at = batch.atom_types.to(dev, torch.int32).contiguous()
    # (with a pool nothing below waits for the device: the times go up from pinned memory, behind the stream's work)
    t_dev = torch.from_numpy(th).to(dev) if pool is None else torch.from_numpy(th).pin_memory().to(dev, non_blocking=True)
    nz = (None, None, None) if noise is None else tuple(f(x) for x in noise)
    yhat = have = None
    if cond is not None and y is not None:
        ya = np.asarray(y.cpu() if torch.is_tensor(y) else y, dtype=np.float64)
        if ya.size != B * model.normalizer.P:
            raise ValueError(f"train_step: y holds {ya.size} values for {B} crystals x {model.normalizer.P} properties")
        up = (lambda a: torch.from_numpy(a).to(dev)) if pool is None else (lambda a: torch.from_numpy(a).pin_memory().to(dev, non_blocking=True))
        yhat, have = (up(a) for a in model.normalizer.normalise(ya))
    model.decoder.sync()
    cb = model.make_batch(na, int(offsets[0]), int(offsets[1]), pool=pool)   # (its own handle: never the module's cache)
    try:
        args = (model.decoder._h, cb._h, _ptr(lengths), _ptr(angles), _ptr(frac0), _ptr(at), _ptr(model.time_embedding.freqs),
                th.ctypes.data_as(C.POINTER(C.c_int)), _ptr(t_dev), _ptr(schedule_table(model)), T, int(seed), int(call_id) & 0xFFFFFFFF,
                _ptr(nz[0]), _ptr(nz[1]), _ptr(nz[2]), model.cost_lattice, model.cost_coord, model.cost_type,
                B if b_global is None else int(b_global), N if n_global is None else int(n_global), int(accum_steps),
                None if forward_only else _ptr(grad), _ptr(stats), _ptr(out_parts))
        if cond is None:
            _lib.check(lib.mi_pretrain_micro_step(*args, _stream()), "mi_pretrain_micro_step")
        else:
            _lib.check(lib.mi_pretrain_micro_step_cond(*args, _ptr(model.prop_freqs), _ptr(yhat), _ptr(have), float(p_uncond), _stream()),
                       "mi_pretrain_micro_step_cond")
    finally:
        # the handle's memory is freed here, which makes the host wait for the micro-step (hipFree waits for the device in any case; the
        # explicit wait on this stream keeps that from resting on the runtime's behaviour)
        # -- a pooled handle frees nothing: its blocks go back to the pool in stream order, and no wait is made
        if pool is None:
            torch.cuda.current_stream().synchronize()
        cb.release()
    return stats


def _as_batch(items, device):
    return CrystalBatchData(list(items)).to(device)


def _shard(items, rank, world):
    """This rank's contiguous shard of a mini-batch: (its items, (first atom, first crystal) in the mini-batch, B and N of the whole)."""
    na = [int(d.num_atoms) for d in items]
    lo, hi = shard_range(len(items), rank, world)
    return items[lo:hi], (sum(na[:lo]), lo), len(na), sum(na), (lo, hi)


def _slice_noise(noise, rows, na_all):
    if noise is None:
        return None
    lo, hi = rows
    n0, n1 = sum(na_all[:lo]), sum(na_all[:hi])
    return noise[0][lo:hi], noise[1][n0:n1], noise[2][n0:n1]


def _eval_enqueue(model, data_list, batch_size, seed, times, acc, pool=None, condition=True):
    """`evaluate` without the read-back: every mini-batch of the set in order, forward-only, normalised by the counts of the WHOLE set (so
    the four sums are the set's losses whatever batch_size is), into the 4 device floats `acc`."""
    n = len(data_list)
    T = model.beta_scheduler.timesteps
    na = [int(d.num_atoms) for d in data_list]
    if times is None:
        tt = draw_times(n, T, 0, 0, seed)
    else:
        if not 1 <= int(times) <= T:
            raise ValueError(f"evaluate: times = {times} lies outside 1..{T}")
        tt = np.full(n, int(times), dtype=np.int32)
    rank, world = rank_world()
    use_y = getattr(model, "condition", None) is not None and bool(condition)
    was_training = model.training
    model.eval()
    try:
        for idx in batch_plan(n, batch_size, 0, seed, shuffle=False):
            lo, hi = shard_range(len(idx), rank, world)
            own = idx[lo:hi]
            if not own:
                continue
            # (the noise is indexed by the crystal's and the atom's position in the SET: the draws do not depend on batch_size either)
            items = [data_list[i] for i in own]
            y = model.normalizer.raw(items) if use_y else None   # (a property-conditioned module: the crystals' values, never dropped; or the null row)
            train_step(model, _as_batch(items, model.device), tt[own], stats=acc, b_global=n, n_global=sum(na), seed=seed,
                       call_id=EVAL_CALL, offsets=(sum(na[:own[0]]), own[0]), forward_only=True, pool=pool, y=y)
    finally:
        model.train(was_training)
    return acc


def evaluate(model, data_list, batch_size, seed=0, times=None, pool=None, condition=True):
    """The four losses of `data_list` under the current weights, forward-only: dict(loss, loss_lattice, loss_coord, loss_type), each the
    mean over ALL elements of the set (mini-batches weighted by their element counts: the result does not depend on batch_size beyond
    fp32 summation order).  times=None: one time per crystal from draw_times(len, T, 0, 0, seed); times=k: every crystal at time k
    (the per-time loss curve).  Noise: Philox at call id 0 under `seed`.  One host read.  pool: train_step's.
    condition (a property-conditioned module): True -- every crystal under its own property values, none dropped; False -- every crystal
    under the null condition (the two losses' difference is what the model has learnt to read from the property)."""
    _refuse(model, "evaluate")
    if int(batch_size) < 1:
        raise ValueError(f"evaluate: batch_size = {batch_size}: must be >= 1")
    if len(data_list) == 0:
        raise ValueError("evaluate: an empty set")
    acc = _eval_enqueue(model, data_list, batch_size, seed, times, torch.zeros(4, device=model.device), pool=pool, condition=condition)
    allreduce_flat_(acc)
    return dict(zip(STATS, acc.tolist()))


def plateau_scheduler(optimizer, spec):
    """cfg.lr_plateau = {factor, patience, min_lr} (all optional: torch's defaults) -> torch.optim.lr_scheduler.ReduceLROnPlateau in 'min'
    mode on `optimizer`; None -> None.  ValueError for any other key."""
    if spec is None:
        return None
    spec = {k: spec[k] for k in spec}
    extra = set(spec) - {"factor", "patience", "min_lr"}
    if extra:
        raise ValueError(f"lr_plateau: unknown key(s) {sorted(extra)}; it takes factor, patience, min_lr")
    kw = {k: v for k, v in spec.items() if v is not None}
    if "patience" in kw:
        kw["patience"] = int(kw["patience"])
    return torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode="min", **kw)


META_KEYS = ("seed", "batch_size", "accum_steps", "shuffle", "n_train", "n_val", "world_size", "T", "numel", "max_grad_norm", "skip_nonfinite",
             "ema_decay", "ema_warmup", "ema_validate", "lr_plateau")


def run_meta(model, optimizer, plateau, seed, batch_size, accum_steps, shuffle, n_train, n_val, ema, condition=None):
    """What decides a run's batch plan, noise and arithmetic besides its weights (META_KEYS): a checkpoint is continued only under the
    same values (check_meta); plus `condition` for a property-conditioned run."""
    o = optimizer.options()
    extra = {} if condition is None else dict(condition=dict(properties=list(condition["properties"]), num_freqs=int(condition["num_freqs"]),
                                                             p_uncond=float(condition["p_uncond"])))
    return dict(extra, seed=int(seed), batch_size=int(batch_size), accum_steps=int(accum_steps), shuffle=bool(shuffle), n_train=int(n_train),
                n_val=int(n_val), world_size=int(rank_world()[1]), T=int(model.beta_scheduler.timesteps), numel=int(model.decoder.theta.numel()),
                max_grad_norm=o["max_grad_norm"], skip_nonfinite=o["skip_nonfinite"], ema_decay=o["ema_decay"], ema_warmup=o["ema_warmup"],
                ema_validate=None if ema is None else bool(ema["validate"]), lr_plateau=plateau is not None)


def check_meta(saved, now):
    """ValueError naming the first key under which the saved run and this one differ: a different batch plan, world size or option would
    silently be a different run."""
    for k in META_KEYS:
        if k not in saved:
            raise ValueError(f"resume: the saved state's meta has no {k}")
        if saved[k] != now[k]:
            raise ValueError(f"resume: {k} = {now[k]!r} in this run, {saved[k]!r} in the saved state")
    # (the condition of a property-conditioned run, DESIGN 41: the key exists in such a run's meta alone, so an unconditional run's meta is META_KEYS)
    if saved.get("condition") != now.get("condition"):
        raise ValueError(f"resume: condition = {now.get('condition')!r} in this run, {saved.get('condition')!r} in the saved state")


def _to_cpu(x):
    if torch.is_tensor(x):
        return x.detach().cpu().clone()
    if isinstance(x, dict):
        return {k: _to_cpu(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_to_cpu(v) for v in x)
    return x


def training_state(model, optimizer, plateau, epoch, history, meta):
    """Everything fit needs to continue a run as the same run, as a plain dict of host copies: the raw weights `theta` (never the
    average), the optimizer's and the plateau scheduler's state_dict, the module's Philox call counter, `epoch` = the next epoch to run,
    the per-epoch history so far and `meta` (run_meta).  Reads the device (one copy per tensor)."""
    return dict(theta=_to_cpu(model.decoder.theta.data), optimizer=_to_cpu(optimizer.state_dict()),
                plateau=None if plateau is None else _to_cpu(plateau.state_dict()), noise_calls=int(getattr(model, "_noise_calls", 0)),
                epoch=int(epoch), history=[dict(d) for d in history], meta=dict(meta))


def save_training_state(path, state, _save=None):
    """Write `state` to `path` through a temporary file in the same directory and os.replace: a job killed in the middle leaves the old
    file (or none), never half of one, and no temporary file.  (_save(obj, file): the writer, torch.save; a test passes one that fails.)"""
    path = os.path.abspath(path)
    fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".tmp", dir=os.path.dirname(path))
    try:
        with os.fdopen(fd, "wb") as f:
            (_save or torch.save)(state, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return path


def load_training_state(path):
    """The inverse of save_training_state, on the host (map_location="cpu")."""
    return torch.load(path, map_location="cpu", weights_only=False)


def _restore(model, optimizer, plateau, state, meta):
    check_meta(state["meta"], meta)
    theta = model.decoder.theta
    with torch.no_grad():
        theta.data.copy_(state["theta"].to(theta.device))
    model.decoder.mark_dirty()
    optimizer.load_state_dict(state["optimizer"])
    if plateau is not None:
        plateau.load_state_dict(state["plateau"])
    model._noise_calls = int(state["noise_calls"])
    return int(state["epoch"]), [dict(d) for d in state["history"]]


def _fit_condition(model, data_list, spec):
    """fit's cfg.condition = {properties: [...], num_freqs: F, p_uncond: 0.1} (guidance.parse_condition) against the module: the module must
    be property-conditioned on exactly these properties and F (ValueError otherwise, and for a condition on an unconditional module or
    none on a conditional one).  Fits the normaliser on the training set (every rank holds the whole set) and leaves it in the module and
    in model.hparams["condition"].  Returns the parsed dict or None."""
    from .guidance import PropertyNormalizer, parse_condition
    cond = parse_condition(spec)
    have = getattr(model, "condition", None)
    if cond is None and have is None:
        return None
    if cond is None:
        raise ValueError("fit: the module is property-conditioned (latent_dim > 0) and the config has no `condition`")
    if have is None or list(have["properties"]) != cond["properties"] or int(have["num_freqs"]) != cond["num_freqs"]:
        raise ValueError(f"fit: condition = {cond['properties']} with num_freqs = {cond['num_freqs']} is not what the module was built for "
                         f"({None if have is None else (have['properties'], have['num_freqs'])}): DiffCSPModule(latent_dim=2 F P, condition=...)")
    nm = PropertyNormalizer(cond["properties"]).fit(data_list)
    if not np.isfinite(nm.raw(data_list)).any():
        raise ValueError(f"fit: no training crystal carries any of the properties {cond['properties']} (CrystalData.properties)")
    model.set_normalizer(nm)
    model.condition["p_uncond"] = model.hparams["condition"]["p_uncond"] = cond["p_uncond"]
    return cond


def fit(model, data_list, cfg, val_list=None, seed=0, noise_fn=None, log=logging.info, on_epoch_end=None, times_fn=None, checkpoint=None,
        resume=None):
    """Train `model` (a DiffCSPModule of the trained grid) on `data_list` (CrystalData records).  cfg (key or attribute access): lr,
    epochs, batch_size; accum_steps (default 1: mini-batches per optimizer step, each normalised by its own counts and 1 / accum_steps);
    shuffle (default true); max_grad_norm / skip_nonfinite_steps (optim.clip_options); lr_plateau = {factor, patience, min_lr}
    (ReduceLROnPlateau on the validation loss, or on the training loss without a validation set); handle_pool = false (default), true or
    {max_bytes: ...}: one pool.HandlePool for the run, behind every mini-batch's handle, closed at the end (pool.parse_handle_pool; its last
    stats() are left in model.handle_pool_stats); ema = null (default), a decay or {decay, warmup: true, validate: true} (optim.parse_ema): the
    optimizer keeps an exponential moving average of the weights in its own pass, with `validate` the validation pass runs on the
    average (FusedAdam.ema_weights: val_loss, and lr_plateau behind it, follow the average) and every epoch dict gains `ema_decay`, the
    decay of the epoch's last step.  The optimizer is then left in model.fit_optimizer (ema_weights for sampling or saving the average).
    checkpoint(epoch, state) runs after on_epoch_end with state = training_state(...) -- at the epochs its optional attribute
    `due(epoch)` accepts, every epoch without one -- and resume=state continues such a run at
    state["epoch"] as the same run, bit for bit: weights, moments, average, the device's step count, learning rate, plateau counters, the
    Philox call counter.  `epochs` may be larger than the saved run's; any other difference (META_KEYS) is a ValueError naming the key.
    The returned history then starts with the loaded epochs.
    One FusedAdam for the whole run; an optimizer step wherever optim.window_closes says so; one host read per epoch (the validation
    pass of `val_list` -- pretrain.evaluate's, same times and noise every epoch -- rides in it).  noise_fn(epoch, step) -> (rand_l,
    rand_x, rand_t) of the whole mini-batch injects the noise and times_fn(epoch, step, B) -> [B] ints in 1..T replaces draw_times (parity
    tests).  on_epoch_end(epoch, stats) runs after every epoch.
    Data parallel: every mini-batch is sharded over the ranks (dist.shard_range) with the whole mini-batch's counts, one flat all-reduce
    precedes each optimizer step, and a rank whose shard is empty still reduces, steps and advances its Philox call id.
    condition = null (default) or {properties: [...], num_freqs: F, p_uncond: 0.1} on a property-conditioned module: the
    normaliser is fitted on the training set and stored in model.hparams["condition"] (a saved model reloads with it), every micro-step
    trains under the crystals' values with the device's condition dropout, the validation pass under the values without dropout, and the
    condition is part of run_meta (a resume under another one is refused by name).
    Returns the list of per-epoch dicts: train_loss, lattice_loss, coord_loss, type_loss (means over the epoch's mini-batches), val_loss,
    val_lattice_loss, val_coord_loss, val_type_loss with a validation set, lr (the epoch's), and the optimizer's grad statistics when it
    clips or guards."""
    from .finetune import _epoch_reduce
    _refuse(model, "fit")
    v = {k: cfg_get(cfg, k) for k in ("lr", "epochs", "batch_size")}
    for k, x in v.items():
        if x is None:
            raise KeyError(f"fit: the config has no {k}")
    lr, epochs, batch_size = float(v["lr"]), int(v["epochs"]), int(v["batch_size"])
    if batch_size < 1:
        raise ValueError(f"fit: batch_size = {batch_size}: must be >= 1")
    if len(data_list) == 0:
        raise ValueError("fit: an empty training set")
    if val_list is not None and len(val_list) == 0:
        raise ValueError("fit: an empty validation set (pass None for no validation)")
    accum = int(cfg_get(cfg, "accum_steps", 1))
    if accum < 1:
        raise ValueError(f"fit: accum_steps = {accum}: must be >= 1")
    shuffle = bool(cfg_get(cfg, "shuffle", True))
    opt = clip_options(cfg)
    pool_kw = parse_handle_pool(cfg_get(cfg, "handle_pool"))
    ema = parse_ema(cfg_get(cfg, "ema"))
    cond = _fit_condition(model, data_list, cfg_get(cfg, "condition"))
    rank, world = rank_world()
    dev = model.device
    theta = model.decoder.theta
    T = model.beta_scheduler.timesteps
    if ema is not None:
        opt = dict(opt, ema_decay=ema["decay"], ema_warmup=ema["warmup"])
    optimizer = FusedAdam([theta], lr=lr, **opt)
    plateau = plateau_scheduler(optimizer, cfg_get(cfg, "lr_plateau"))
    if theta.grad is None:
        theta.grad = torch.zeros_like(theta)
    n = len(data_list)
    out, first, meta = [], 0, None
    if checkpoint is not None or resume is not None:
        meta = run_meta(model, optimizer, plateau, seed, batch_size, accum, shuffle, n, 0 if val_list is None else len(val_list), ema, cond)
    if resume is not None:
        first, out = _restore(model, optimizer, plateau, resume, meta)
    if ema is not None:
        model.__dict__["fit_optimizer"] = optimizer
    pool = None if pool_kw is None else HandlePool(**pool_kw)
    try:
        return _fit_epochs(model, data_list, val_list, seed, noise_fn, log, on_epoch_end, times_fn, epochs, batch_size, accum, shuffle, optimizer,
                           plateau, pool, out, first, ema, checkpoint, meta, cond)
    finally:
        if pool is not None:
            model.__dict__["handle_pool_stats"] = pool.stats()   # (the run's pool just before it is closed: HandlePool.stats())
            pool.close()


def _fit_epochs(model, data_list, val_list, seed, noise_fn, log, on_epoch_end, times_fn, epochs, batch_size, accum, shuffle, optimizer, plateau, pool, out,
                first=0, ema=None, checkpoint=None, meta=None, cond=None):
    """fit's epoch loop (its docstring); `pool`: the run's HandlePool or None; `first`: the epoch to start at; `ema`: parse_ema's dict."""
    from .finetune import _epoch_reduce
    rank, world = rank_world()
    dev = model.device
    theta = model.decoder.theta
    T = model.beta_scheduler.timesteps
    n = len(data_list)
    for epoch in range(first, epochs):
        model.train()
        optimizer.zero_grad(set_to_none=False)
        acc = torch.zeros(4, device=dev)
        plan = batch_plan(n, batch_size, epoch, seed, shuffle)
        for step, idx in enumerate(plan):
            items = [data_list[i] for i in idx]
            own, offsets, b_glob, n_glob, rows = _shard(items, rank, world)
            model._noise_calls = getattr(model, "_noise_calls", 0) + 1   # one call id per micro-step, on every rank
            if own:
                noise = None if noise_fn is None else _slice_noise(noise_fn(epoch, step), rows, [int(d.num_atoms) for d in items])
                times = draw_times(len(idx), T, epoch, step, seed) if times_fn is None else np.asarray(times_fn(epoch, step, len(idx)))
                kw = {} if cond is None else dict(y=model.normalizer.raw(own), p_uncond=cond["p_uncond"])
                train_step(model, _as_batch(own, dev), times[rows[0]:rows[1]], noise=noise, grad=theta.grad,
                           stats=acc, b_global=b_glob, n_global=n_glob, accum_steps=accum, seed=seed, call_id=model._noise_calls, offsets=offsets,
                           pool=pool, **kw)
            if window_closes(step + 1, accum, len(plan)):
                allreduce_flat_(theta.grad)
                optimizer.step()
                optimizer.zero_grad(set_to_none=False)
        if val_list is not None:
            # (with ema.validate the set's loss is the average's: one exchange and one re-pack of the weights each way, all enqueued)
            with optimizer.ema_weights(model.decoder) if ema is not None and ema["validate"] else contextlib.nullcontext():
                acc = torch.cat([acc, _eval_enqueue(model, val_list, batch_size, seed, None, torch.zeros(4, device=dev), pool=pool)])
        k_ema = None
        if ema is not None and optimizer.guarded:   # the applied-step count rides in the epoch's read (rank 0's: the ranks agree)
            k_ema = acc.numel()
            s_dev = optimizer.adam_steps()
            acc = torch.cat([acc, s_dev if rank == 0 else torch.zeros_like(s_dev)])
        a = _epoch_reduce(acc, "fit", optimizer)   # the epoch's only host read
        s_ema = None
        if k_ema is not None:
            s_ema = int(round(a.pop(k_ema)))
        elif ema is not None:
            s_ema = int(optimizer.state[theta]["step"])
        d = dict(train_loss=a[0] / len(plan), lattice_loss=a[1] / len(plan), coord_loss=a[2] / len(plan), type_loss=a[3] / len(plan))
        k = 4
        if val_list is not None:
            d.update(val_loss=a[4], val_lattice_loss=a[5], val_coord_loss=a[6], val_type_loss=a[7])
            k = 8
        d["lr"] = float(optimizer.param_groups[0]["lr"])
        if len(a) > k:
            d.update(epoch_grad_stats(a[k:]))
        if ema is not None:
            d["ema_decay"] = ema_decay_at(ema["decay"], ema["warmup"], s_ema)
        if plateau is not None:
            plateau.step(d["val_loss"] if val_list is not None else d["train_loss"])
        out.append(d)
        if rank == 0:
            log(f"Epoch {epoch}: " + ", ".join(f"{k_}: {v_:.6g}" for k_, v_ in d.items()))
        if on_epoch_end is not None:
            on_epoch_end(epoch, d)
        if checkpoint is not None and getattr(checkpoint, "due", lambda e: True)(epoch):   # (`due`: the state is copied off the device only then)
            checkpoint(epoch, training_state(model, optimizer, plateau, epoch + 1, out, meta))
    return out

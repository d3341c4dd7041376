"""DiffCSP diffusion module on the HIP path.

Mirror of models/diffcsp/diffusion.py:69-399 (DiffCSPModule): same constructor hparams,
same buffers (`beta_scheduler.*`, `sigma_scheduler.*`), same methods
`sample / add_noise / calc_sample_loss / calc_kl_reg`, same `decoder.*` parameter names in
`state_dict()`.  The arithmetic runs in libmatinvent_hip.so; there is no PyTorch fallback.
"""
import contextlib
import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from .cspnet import CSPNet, CrystalBatch, MAX_ATOMIC_NUM, _ptr, _stream
from .schedules import (BetaScheduler, SigmaScheduler, respaced_schedulers, respaced_times, sampler_coefficients,
                        time_embedding_freqs)


def _scatter_mean(src, index, dim_size):
    """torch_scatter.scatter(..., reduce='mean') on the device: sum / max(count, 1)."""
    out = torch.zeros(dim_size, dtype=src.dtype, device=src.device).index_add(0, index, src)
    cnt = torch.zeros(dim_size, dtype=src.dtype, device=src.device).index_add(0, index, torch.ones_like(src))
    return out / cnt.clamp(min=1)


def p_wrapped_normal(x, sigma, N=10, T=1.0):
    """diffusion.py:18-22 (host utility: the device kernels carry their own copy of the sum)."""
    p_ = 0
    for i in range(-N, N + 1):
        p_ += torch.exp(-(x + T * i) ** 2 / 2 / sigma ** 2)
    return p_


def log_prob_wn(x, mu, sigma, N=10, T=1.0):
    """diffusion.py:25-29: log of the naive 21-image wrapped-normal sum (host utility; csrc/logprob.h is the device form)."""
    p_ = 0
    for i in range(-N, N + 1):
        p_ += torch.exp(-(x - mu + T * i) ** 2 / 2 / sigma ** 2)
    return torch.log(p_)


def _cfg(d, drop=("_target_",)):
    return {k: v for k, v in dict(d).items() if k not in drop}


class SinusoidalTimeEmbeddings(nn.Module):
    """diffusion.py:53-66, evaluated on the device from the host-built frequency table."""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim
        self.register_buffer("freqs", time_embedding_freqs(dim), persistent=False)

    def forward(self, time):
        lib = _lib.load()
        times = time.to(self.freqs.device, torch.int32).contiguous()
        out = torch.empty(times.shape[0], self.dim, device=self.freqs.device)
        _lib.check(lib.mi_time_embedding(_ptr(times), _ptr(self.freqs), times.shape[0], self.dim, _ptr(out), _stream()))
        return out


class _Counts:
    """Atom counts of a contiguous group of crystals (what `sample` needs of a batch)."""

    def __init__(self, num_atoms):
        self.num_atoms = torch.as_tensor(num_atoms, dtype=torch.long)


class _TrajPair:
    """The corrector's and the predictor's batch handle of forward_logprb for one atom-count vector, and the number of calls made on them
    (a taped call's backward runs only while it is the latest: the C entry's MI_ESTATE check sees evaluations of the handles, this counter
    sees which forward_logprb call left them)."""

    def __init__(self, b_corr, b_pred):
        self.handles = (b_corr, b_pred)
        self.calls = 0


class DiffCSPModule(nn.Module):
    def __init__(self, decoder, beta_scheduler, sigma_scheduler, latent_dim=0, time_dim=256, cost_lattice=1.0,
                 cost_coord=1.0, cost_type=20.0, device=None, **kwargs):
        super().__init__()
        self.hparams = dict(decoder=dict(decoder), beta_scheduler=dict(beta_scheduler), sigma_scheduler=dict(sigma_scheduler),
                            latent_dim=latent_dim, time_dim=time_dim, cost_lattice=cost_lattice, cost_coord=cost_coord,
                            cost_type=cost_type, **kwargs)
        dev = torch.device(device if device is not None else "cuda")
        # diffusion.py:73 -- latent_dim + time_dim, pred_type=True, smooth=True
        self.decoder = CSPNet(**_cfg(decoder), latent_dim=latent_dim + time_dim, pred_type=True, smooth=True, device=dev)
        self.beta_scheduler = BetaScheduler(**_cfg(beta_scheduler))
        self.sigma_scheduler = SigmaScheduler(**_cfg(sigma_scheduler))
        self.time_dim = time_dim
        self.time_embedding = SinusoidalTimeEmbeddings(time_dim)
        self.cost_lattice, self.cost_coord, self.cost_type = cost_lattice, cost_coord, cost_type
        self.keep_lattice = cost_lattice < 1e-5   # diffusion.py:78-79: CSP mode, that part of the structure is given
        self.keep_coords = cost_coord < 1e-5
        self._init_condition(kwargs.get("condition"), latent_dim)
        self.to(dev)

    # ---- property-conditioned prior (guidance.py) ---------------------------------------
    condition = None    # guidance.parse_condition's dict of a module with a property part (latent_dim = 2 F P); None: the unconditional prior
    normalizer = None   # ... and its guidance.PropertyNormalizer (mean 0, std 1 until pretrain.fit has fitted it)

    def _init_condition(self, spec, latent_dim):
        """latent_dim > 0 takes hparams `condition` = {properties, num_freqs[, p_uncond, mean, std]} with 2 F P = latent_dim and records the
        layout on the network (mi_net_set_latent: every fused entry then fills or refuses the property columns); latent_dim = 0 takes none."""
        from . import guidance
        cond = guidance.parse_condition(spec)
        if cond is None and not latent_dim:
            return
        if cond is None or not latent_dim or guidance.latent_dim(len(cond["properties"]), cond["num_freqs"]) != int(latent_dim):
            raise ValueError(f"DiffCSPModule: latent_dim = {latent_dim} and condition = {spec!r} do not go together: a property-conditioned prior has "
                             "condition = {properties: [P names], num_freqs: F} and latent_dim = 2 F P, an unconditional one neither")
        _lib.check(_lib.load().mi_net_set_latent(self.decoder._h, len(cond["properties"]), cond["num_freqs"]), "mi_net_set_latent")
        self.condition = cond
        self.normalizer = guidance.PropertyNormalizer(cond["properties"], cond.get("mean"), cond.get("std"))
        self.register_buffer("prop_freqs", guidance.property_freqs(cond["num_freqs"]), persistent=False)

    def set_normalizer(self, normalizer):
        """Adopt a fitted PropertyNormalizer (pretrain.fit): into the module and into hparams["condition"], so that a saved model reloads with it."""
        if self.condition is None or list(normalizer.names) != list(self.condition["properties"]):
            raise ValueError("set_normalizer: the normaliser's properties are not the module's")
        self.normalizer = normalizer
        self.condition = dict(self.condition, **{k: v for k, v in normalizer.to_dict().items() if k != "properties"})
        self.hparams["condition"] = dict(self.condition)

    def _yhat(self, y, B, where):
        """(yhat, have) device tensors [B][P] of raw property values `y` ([B][P] or [B] for P = 1; NaN: missing), or (None, None)."""
        if y is None:
            return None, None
        import numpy as np
        a = np.asarray(y.cpu() if torch.is_tensor(y) else y, dtype=np.float64)
        nm = (self.base if self.base is not None else self).normalizer   # (a view made before fit fitted it reads the module's)
        if a.size != B * nm.P:
            raise ValueError(f"{where}: y holds {a.size} values for {B} crystals x {nm.P} properties")
        yhat, have = nm.normalise(a)
        return torch.from_numpy(yhat).to(self.device), torch.from_numpy(have).to(self.device)

    def crystal_embedding(self, times, y=None, drop=None):
        """[B][time_dim + Z]: the embedding rows the network of a property-conditioned prior reads (mi_crystal_embedding) at the per-crystal
        `times` -- the time embedding, then per property sin / cos of w_k clamp(y^); y: raw property values [B][P] (NaN: missing), None: the
        null row for every crystal; drop: [B] bool, the crystals whose condition is dropped.  On a respaced view `times` are step indices."""
        from . import guidance
        guidance.module_condition(self, "crystal_embedding")
        dev = self.device
        times = torch.as_tensor(times).to(dev, torch.int32).contiguous().reshape(-1)
        B = times.shape[0]
        yhat, have = self._yhat(y, B, "crystal_embedding")
        dr = None if drop is None else torch.as_tensor(drop).to(dev).reshape(-1).to(torch.int32).contiguous()
        if dr is not None and dr.shape[0] != B:
            raise ValueError(f"crystal_embedding: drop holds {dr.shape[0]} entries for {B} crystals")
        out = torch.empty(B, self.decoder.latent_dim, device=dev)
        cb = None
        if self.time_map is not None:   # (a view: the map rides on a handle, and the entry reads nothing else of it -- the view's one-atom handle serves every B)
            cb = self._batch_for(torch.ones(1, dtype=torch.long))
        _lib.check(_lib.load().mi_crystal_embedding(self.decoder._h, None if cb is None else cb._h, B, _ptr(times), 0, _ptr(self.time_embedding.freqs),
                                                    _ptr(self.prop_freqs), _ptr(yhat), _ptr(have), _ptr(dr), _ptr(out), _stream()), "mi_crystal_embedding")
        return out

    @property
    def device(self):
        return self.decoder.theta.device

    # ---- strided reverse chain ---------------------------------------------------------
    base = None       # a view made by `respaced`: the module it shares its decoder with
    time_map = None   # ... and its grid tau_0 .. tau_S (host int32 [S + 1]); None on a module of the trained grid

    def respaced(self, steps=None, times=None):
        """A light view of this module whose reverse chain runs on S of the T trained steps: `steps` = S on the default grid
        tau_k = (2 k T + S) // (2 S), or `times` = an explicit grid (schedules.respaced_times).  The view SHARES the decoder (the same
        theta: gradients and optimiser steps through the view land in this module), the time-embedding frequencies, the keep flags and
        the costs; it has its OWN re-spaced schedulers (timesteps = S; schedules.respaced_schedulers), coefficient tables and batch
        handles, and carries `.base` (this module) and `.time_map` (tau, int32 [S + 1]).  The full grid -- respaced(T), times = 0..T --
        is this module itself.  Views are kept per grid until a scheduler buffer changes (checkpoint load).

        On a view every `t`, `t_start`, `t_stop`, `timesteps`, record index and the noise stream's step field is a STEP INDEX k in
        0..S (the initial draw uses S + 1): a strided chain's noise is keyed by step index, so the chains of two grids from one seed
        share their initial state and nothing else.  The network alone sees the trained time tau_k, through the map every batch
        handle of the view carries (mi_batch_set_time_map).  sample / forward_logprb / sampling.* / policy.pg_step take a view;
        the fine-tune surface (add_noise, calc_sample_loss, calc_kl_reg) belongs to the trained grid: use `.base`."""
        if self.base is not None:
            raise ValueError("respaced: this module is a strided view already; re-space its .base")
        T = self.beta_scheduler.timesteps
        tau = respaced_times(T, steps, times)
        if len(tau) == T + 1:
            return self
        key = (tuple(tau),) + tuple(b._version for b in (self.beta_scheduler.alphas_cumprod, self.sigma_scheduler.sigmas,
                                                          self.sigma_scheduler.sigmas_norm))
        cache = self.__dict__.setdefault("_respaced", {})
        view = cache.get(key)
        if view is None:
            for k in [k for k in cache if k[0] == key[0]]:
                del cache[k]
            if len(cache) >= 4:
                cache.pop(next(iter(cache)))
            view = DiffCSPModule.__new__(DiffCSPModule)
            nn.Module.__init__(view)
            view.hparams = self.hparams
            view.decoder = self.decoder
            view.beta_scheduler, view.sigma_scheduler = respaced_schedulers(self.beta_scheduler, self.sigma_scheduler, tau)
            view.time_dim, view.time_embedding = self.time_dim, self.time_embedding
            view.cost_lattice, view.cost_coord, view.cost_type = self.cost_lattice, self.cost_coord, self.cost_type
            view.keep_lattice, view.keep_coords = self.keep_lattice, self.keep_coords
            if self.condition is not None:
                view.condition, view.normalizer = self.condition, self.normalizer
                view.register_buffer("prop_freqs", self.prop_freqs, persistent=False)
            view.time_map = torch.tensor(tau, dtype=torch.int32)
            object.__setattr__(view, "base", self)   # (not a submodule of its own view)
            view.train(self.training)
            cache[key] = view
        return view

    def make_batch(self, num_atoms, node_offset=0, graph_offset=0, pool=None) -> CrystalBatch:
        """A batch handle of the decoder for THIS module's chain: a strided view's handles carry its time map (set here, once, at creation).
        pool: a pool.HandlePool the handle's memory is taken from (training handles of the trained grid)."""
        cb = self.decoder.make_batch(num_atoms, node_offset, graph_offset, pool=pool)
        if self.time_map is not None:
            tm = self.time_map.numpy()
            _lib.check(_lib.load().mi_batch_set_time_map(cb._h, tm.ctypes.data_as(C.POINTER(C.c_int)), len(tm)), "mi_batch_set_time_map")
        return cb

    def _coefficients(self, step_lr):
        """Per-step scalar table, cached until a scheduler buffer changes (checkpoint load)."""
        key = (float(step_lr),) + tuple(b._version for b in (self.beta_scheduler.alphas, self.beta_scheduler.alphas_cumprod,
                                                              self.beta_scheduler.sigmas, self.sigma_scheduler.sigmas,
                                                              self.sigma_scheduler.sigmas_norm))
        cache = self.__dict__.setdefault("_coef_cache", {})
        if key not in cache:
            cache.clear()
            cache[key] = sampler_coefficients(self.beta_scheduler, self.sigma_scheduler, step_lr).contiguous()
        return cache[key]

    def crystal_batch(self, batch, node_offset=0, graph_offset=0) -> CrystalBatch:
        """Index tables + workspace for `batch` (anything with .num_atoms); cached on the object
        PER MODULE (agent and frozen prior must not share workspace: a forward of one would
        clobber the activations the other's pending backward reads)."""
        cache = getattr(batch, "_mi_batches", None)
        if cache is None:
            cache = {}
            try:
                batch._mi_batches = cache
            except AttributeError:
                pass
        key = (id(self), node_offset, graph_offset)
        cb = cache.get(key)
        if cb is None or cb.num_atoms_list != [int(x) for x in batch.num_atoms.tolist()]:
            cb = self.make_batch(batch.num_atoms, node_offset, graph_offset)
            cache[key] = cb
        return cb

    # ---- fine-tune surface (pipeline/mat_invent.py:152-161) ------------------------------------
    def add_noise(self, batch, time=None, noise=None, seed=None, times=None, y=None, drop=None):
        """DiffCSPModule.add_noise (diffusion.py:81-119) for an explicit timestep index
        (`time` in 0..T-1 -> diffusion time T - time, :86-87).  Returns the reference's triple
        (noised_input, noises, batch.batch).  Fresh Gaussian noise per call from the Philox
        stream (seed, running call counter) unless `noise` = (rand_l, rand_x, rand_t).
        `times` (with time=None): the per-crystal diffusion times, [B] ints in 1..T, in place of the numpy draw.
        On a property-conditioned module the first element of noised_input is the crystal embedding (crystal_embedding): under the raw
        property values `y` with the crystals of `drop` left without, or -- y = None -- the null row."""
        lib = _lib.load()
        dev = self.device
        T = self.beta_scheduler.timesteps
        cb = self._batch_for(batch.num_atoms)
        B, N = cb.num_graphs, cb.num_nodes
        sched = None
        if time is not None and times is not None:
            raise ValueError("add_noise: give `time` (one index for every crystal) or `times` (one time per crystal), not both")
        if time is None:   # :83-84: one uniformly drawn time per crystal (numpy's global generator, like the reference)
            if times is None:
                times = self.beta_scheduler.uniform_sample_t(B, dev)
            else:
                times = torch.as_tensor(times).long().reshape(-1)
                if times.numel() != B or (B and (int(times.min()) < 1 or int(times.max()) > T)):
                    raise ValueError(f"add_noise: `times` must hold {B} values in 1..{T}")
                times = times.to(dev)
            ac = self.beta_scheduler.alphas_cumprod[times]
            sched = torch.stack([torch.sqrt(ac), torch.sqrt(1.0 - ac), self.sigma_scheduler.sigmas[times],
                                 self.sigma_scheduler.sigmas_norm[times]], dim=1).to(torch.float32).contiguous()
        else:
            t = T - int(time)
            times = torch.full((B,), t, device=dev)
            ac = self.beta_scheduler.alphas_cumprod[t]
            c0, c1 = float(torch.sqrt(ac)), float(torch.sqrt(1.0 - ac))
            sig, sn = float(self.sigma_scheduler.sigmas[t]), float(self.sigma_scheduler.sigmas_norm[t])
        if self.condition is not None:
            time_emb = self.crystal_embedding(times, y, drop)
        elif y is not None or drop is not None:
            raise ValueError("add_noise: y / drop need a property-conditioned module (latent_dim > 0)")
        else:
            time_emb = self.time_embedding(times)
        f = lambda x: x.to(dev, torch.float32).contiguous()
        lengths, angles, frac0 = f(batch.lengths), f(batch.angles), f(batch.frac_coords)
        at = batch.atom_types.to(dev, torch.int32).contiguous()
        in_lat, in_frac = torch.empty(B, 3, 3, device=dev), torch.empty(N, 3, device=dev)
        in_types, tar_x = torch.empty(N, MAX_ATOMIC_NUM, device=dev), torch.empty(N, 3, device=dev)
        rand_l, rand_t = torch.empty(B, 3, 3, device=dev), torch.empty(N, MAX_ATOMIC_NUM, device=dev)
        nz = (None, None, None) if noise is None else tuple(f(x) for x in noise)
        self._noise_calls = getattr(self, "_noise_calls", 0) + 1
        seed = getattr(self, "noise_seed", 0) if seed is None else seed
        if sched is not None:
            _lib.check(lib.mi_add_noise_per_crystal(cb._h, _ptr(lengths), _ptr(angles), _ptr(frac0), _ptr(at), _ptr(sched), seed,
                                                    self._noise_calls & 0xFFFFFFFF, _ptr(nz[0]), _ptr(nz[1]), _ptr(nz[2]), _ptr(in_lat),
                                                    _ptr(in_frac), _ptr(in_types), _ptr(tar_x), _ptr(rand_l), _ptr(rand_t), _stream()),
                       "mi_add_noise_per_crystal")
        else:
            _lib.check(lib.mi_add_noise(cb._h, _ptr(lengths), _ptr(angles), _ptr(frac0), _ptr(at), c0, c1, sig, sn, seed,
                                        self._noise_calls & 0xFFFFFFFF, _ptr(nz[0]), _ptr(nz[1]), _ptr(nz[2]), _ptr(in_lat), _ptr(in_frac),
                                        _ptr(in_types), _ptr(tar_x), _ptr(rand_l), _ptr(rand_t), _stream()), "mi_add_noise")
        noised_input = (time_emb, in_types, in_frac, in_lat, cb.num_atoms, cb.batch)
        return noised_input, (rand_l, tar_x, rand_t), cb.batch

    def predict(self, input_all):
        """The network evaluation of calc_sample_loss alone (diffusion.py:124-125): library kernels only, no torch arithmetic -- the part
        that may run on a side stream beside another network's forward (finetune._surface_timestep)."""
        noised_input, _, node2graph = input_all
        time_emb, atom_types, frac, lattices, num_atoms, _ = noised_input
        return self.decoder(time_emb, atom_types, frac, lattices, num_atoms, node2graph, batch=self._batch_for(num_atoms))

    def calc_sample_loss(self, input_all, pred=None):
        """diffusion.py:121-138: per-crystal cost_lattice*mse_l + cost_coord*mse_x + cost_type*mse_t (`pred`: the output of `predict`,
        when the caller has run the network already)."""
        noised_input, (rand_l, tar_x, rand_t), node2graph = input_all
        time_emb, atom_types, frac, lattices, num_atoms, _ = noised_input
        B = lattices.shape[0]
        pred_l, pred_x, pred_t = pred if pred is not None else self.predict(input_all)
        loss_lattice = torch.pow(pred_l - rand_l, 2).mean(dim=(1, 2))
        loss_coord = _scatter_mean(torch.pow(pred_x - tar_x, 2).mean(dim=1), node2graph, B)
        loss_type = _scatter_mean(torch.pow(pred_t - rand_t, 2).mean(dim=1), node2graph, B)
        loss = self.cost_lattice * loss_lattice + self.cost_coord * loss_coord + self.cost_type * loss_type
        return loss, (pred_l, pred_x, pred_t)

    def calc_kl_reg(self, agent_pred, prior_pred, batch):
        """diffusion.py:140-149: per-crystal sum of three mean-squared agent-prior differences."""
        pl, px, pt = agent_pred
        plp, pxp, ptp = (p.detach() for p in prior_pred)
        node2graph = batch.batch if hasattr(batch, "batch") else batch
        node2graph = node2graph.to(pl.device)
        B = pl.shape[0]
        k0 = torch.pow(pl - plp, 2).mean(dim=(1, 2))
        k1 = _scatter_mean(torch.pow(px - pxp, 2).mean(dim=1), node2graph, B)
        k2 = _scatter_mean(torch.pow(pt - ptp, 2).mean(dim=1), node2graph, B)
        return k0 + k1 + k2

    def training_step(self, batch, times=None, noise=None, y=None, drop=None):
        """DiffCSPModule.training_step (diffusion.py:457-486) on the module surface: add_noise with one time per crystal (`times`: [B]
        ints in 1..T in place of the numpy draw), the network, three F.mse_loss over all elements of the batch, the cost-weighted sum.
        Returns (loss, dict(loss, loss_lattice, loss_coord, loss_type)); differentiable through the decoder's autograd function.  The
        unfused yardstick of pretrain.train_step, as ft_step(fused=False) is of the fused fine-tune step."""
        if self.base is not None:
            raise ValueError("training_step: a respaced view is for sampling; train its .base, the module of the trained grid")
        input_all = self.add_noise(batch, None, noise=noise, times=times, y=y, drop=drop)   # (y, drop: add_noise's, a property-conditioned module)
        _, (rand_l, tar_x, rand_t), _ = input_all
        pred_l, pred_x, pred_t = self.predict(input_all)
        mse = nn.functional.mse_loss
        loss_lattice, loss_coord, loss_type = mse(pred_l, rand_l), mse(pred_x, tar_x), mse(pred_t, rand_t)
        loss = self.cost_lattice * loss_lattice + self.cost_coord * loss_coord + self.cost_type * loss_type
        return loss, dict(loss=loss, loss_lattice=loss_lattice, loss_coord=loss_coord, loss_type=loss_type)

    def forward(self, noised_input):
        time_emb, atom_types, frac, lattices, num_atoms, node2graph = noised_input
        return self.decoder(time_emb, atom_types, frac, lattices, num_atoms, node2graph, batch=self._batch_for(num_atoms))

    # ---- trajectory log-probabilities (diffusion.py:158-227) ------------------------------------
    def _traj_batches(self, num_atoms):
        """The (corrector, predictor) pair of batch handles forward_logprb evaluates on: its own, per atom-count vector, apart from
        `crystal_batch` / `_batch_for` -- a call never overwrites a fine-tune tape or a weight-gradient window."""
        key = tuple(int(x) for x in num_atoms.tolist())
        cache = self.__dict__.setdefault("_traj_cache", {})
        pair = cache.get(key)
        if pair is None:
            if len(cache) >= 4:
                cache.pop(next(iter(cache)))
            pair = _TrajPair(self.make_batch(list(key)), self.make_batch(list(key)))
            cache[key] = pair
        pair.calls += 1   # every call overwrites what the pair holds: a pending backward of an earlier call must refuse (TrajLogProbFunction)
        return pair

    def forward_logprb(self, state, step_lr=1e-5, condition=None, likelihood=None):
        """DiffCSPModule.forward_logprb (diffusion.py:158-227): re-evaluate one recorded step -- the corrector's network evaluation on
        (atom_types, frac_coords, lattices), the predictor's on frac_coords_mid -- under the current weights.  Returns
        (log_prob_l, log_prob_t, log_prob_x, (pred_l_corr, pred_x_corr, pred_t_corr)) like the reference, differentiable with respect
        to decoder.theta when grad is enabled (matinvent_amd.autograd.TrajLogProbFunction); under torch.no_grad() nothing is taped.

        Deviation: crystal b is evaluated at ITS OWN timesteps[b] (time embedding and scalars); the reference takes timesteps[0]'s scalars
        for every crystal.  The two agree whenever the timesteps are equal -- the only case sample_mdp produces.  t must lie in 2..T
        (ValueError otherwise; the reference's formulas give inf / NaN at t = 1).  One pending backward per atom-count vector: a later
        call with the same atom counts overwrites the tapes, and the earlier call's backward then raises instead of returning wrong
        gradients.  A `condition` alone is refused (ValueError): the unmasked sums are not a conditioned chain's likelihood.
        condition=c, likelihood="free" (DESIGN 36): `state` is a step of a chain sampled under `c` (for the crystals of `state`), and the
        predictor terms of c's known elements leave the three log-probabilities and their gradients -- the trajectory likelihood of the
        conditioned chain up to a constant of theta.  The handle pair carries c's masks for the call alone (one device synchronisation)."""
        from .conditioning import check_likelihood
        from .guidance import refuse_latent
        refuse_latent(self, "forward_logprb")
        masked = check_likelihood("forward_logprb", likelihood, condition)
        if condition is not None and not masked:
            raise ValueError("forward_logprb: a condition is not supported -- the recorded log-probabilities of a conditioned chain are those "
                             "of the unconditioned proposal, not a trajectory likelihood")
        for k, v in state.items():   # (the reference moves the caller's tensors to the device in place, :159-160)
            state[k] = v.to(self.device)
        T = self.beta_scheduler.timesteps
        times = state["timesteps"].to(torch.int32)
        th = times.cpu()
        if th.numel() and (int(th.min()) < 2 or int(th.max()) > T):
            raise ValueError(f"forward_logprb: timesteps must lie in 2..{T} (got {int(th.min())}..{int(th.max())}); the reference's "
                             "formulas give inf / NaN at t = 1")
        num_atoms = state["num_atoms"]
        if masked and [int(v) for v in condition.num_atoms.tolist()] != [int(v) for v in num_atoms.tolist()]:
            raise ValueError("forward_logprb: the condition's atom counts are not the state's")
        pair = self._traj_batches(num_atoms)
        batches = pair.handles
        with self._conditioned([(cb, condition) for cb in batches] if masked else [], condition=False, likelihood=masked):
            return self._forward_logprb(state, step_lr, pair, times, T)

    def _forward_logprb(self, state, step_lr, pair, times, T):
        """forward_logprb after its checks, on the handle pair `pair` (which carries a likelihood mask or none)."""
        dev = self.device
        batches = pair.handles
        B, N = batches[0].num_graphs, batches[0].num_nodes
        f = lambda k: state[k].detach().to(dev, torch.float32).contiguous()
        at, fr, fm, lat = f("atom_types"), f("frac_coords"), f("frac_coords_mid"), f("lattices")
        nat, nfr, nlat = f("next_atom_types"), f("next_frac_coords"), f("next_lattices")
        assert at.shape == (N, MAX_ATOMIC_NUM) and fr.shape == fm.shape == nfr.shape == (N, 3) and lat.numel() == nlat.numel() == B * 9
        coef = self._coefficients_dev(step_lr)
        times = times.to(dev).contiguous()
        freqs = self.time_embedding.freqs
        theta = self.decoder.theta
        if torch.is_grad_enabled() and theta.requires_grad:
            from .autograd import TrajLogProbFunction
            lp_l, lp_t, lp_x, pl, px, pt = TrajLogProbFunction.apply(theta, self.decoder, pair, times, coef, T, freqs, at, fr, fm, lat,
                                                                     nat, nfr, nlat)
            return lp_l, lp_t, lp_x, (pl, px, pt)
        lib = _lib.load()
        self.decoder.sync()
        lp = torch.empty(3, B, device=dev)
        pl, px, pt = torch.empty(B, 3, 3, device=dev), torch.empty(N, 3, device=dev), torch.empty(N, MAX_ATOMIC_NUM, device=dev)
        _lib.check(lib.mi_traj_logprob(self.decoder._h, batches[0]._h, batches[1]._h, _ptr(times), _ptr(coef), T, _ptr(freqs), _ptr(at),
                                       _ptr(fr), _ptr(fm), _ptr(lat), _ptr(nat), _ptr(nfr), _ptr(nlat), _ptr(lp), _ptr(pl), _ptr(px), _ptr(pt),
                                       0, _stream()), "mi_traj_logprob")
        return lp[0], lp[1], lp[2], (pl, px, pt)

    def _coefficients_dev(self, step_lr):
        """_coefficients on the device (mi_traj_logprob reads the table there), cached with it."""
        host = self._coefficients(step_lr)
        cached = self.__dict__.get("_coef_dev")
        if cached is None or cached[0] is not host or cached[1].device != self.device:
            cached = (host, host.to(self.device).contiguous())
            self.__dict__["_coef_dev"] = cached
        return cached[1]

    def _batch_for(self, num_atoms):
        """CrystalBatch of THIS module for a num_atoms tensor (small cache keyed by the atom counts and
        the shard offsets `self.shard_offsets` = (first global atom, first global crystal), which only
        enter the noise counters)."""
        off = getattr(self, "shard_offsets", (0, 0))
        key = (tuple(int(x) for x in num_atoms.tolist()), off)
        cache = self.__dict__.setdefault("_nb_cache", {})
        cb = cache.get(key)
        if cb is None:
            if len(cache) >= 8:
                cache.pop(next(iter(cache)))
            cb = self.make_batch(list(key[0]), off[0], off[1])
            cache[key] = cb
        return cb

    @torch.no_grad()
    def sample(self, batch, diff_ratio=1.0, step_lr=1e-5, seed=0, noise=None, init=None, record=False, t_start=None,
               t_stop=0, node_offset=0, graph_offset=0, streams=None, rec_sink=None, condition=None, likelihood=None, resample=None,
               guidance=None, steer=None, classifier=None, symmetry=None):
        """DiffCSPModule.sample (diffusion.py:273-399).

        `rec_sink` (a list; with record=True): receives one (first crystal, first atom, buffers) per chain, in crystal order -- the
        chain's stacked record buffers [T+1, ...] (atom_types, frac_coords, lattices, frac_coords_mid, log_prob_{l,t,x}) that the
        per-step dict `traj` views (sampling.sample_rollout compacts them on the device).

        `streams` > 1 splits the crystals into that many contiguous groups and runs their chains CONCURRENTLY on separate
        HIP streams (crystals never interact, and the counter-based noise is indexed by global atom / crystal id, so the
        samples are the same as those of the unsplit batch): the node-level kernels and the partial last round of one
        group's edge GEMMs overlap the other groups' edge GEMMs.  None = automatic (2-4 for large batches).

        On a strided view (`respaced`) T is the view's S and t_start / t_stop / the keys of `traj` / the first index of `noise` and of the
        record buffers are step indices 0..S; the counter-based noise is keyed by step index (initial draw: S + 1).

        `condition` (conditioning.Condition for the crystals of `batch`; it may BE `batch`): replacement conditioning.  The known
        atom types / coordinates / lattices are overwritten at the start and after every step with a forward-noised copy of their clean
        values at the level the chain has reached (on a view: the step index, through the view's tables), and are exact at t_stop = 0.  The
        condition is attached to the chain's batch handles for this call and cleared afterwards (one device synchronisation before the
        call's first launch, none inside the chain).  With record=True the CONDITIONED states are recorded; the recorded log-probabilities
        are then those of the unconditioned proposal of each step -- not a trajectory likelihood, which is why sample_mdp, sample_rollout
        and forward_logprb refuse a condition.  CSP mode together with a condition is refused by the library (MI_EINVAL).

        `likelihood` = "free" (with a condition): the chain's handles also carry the condition's masks as their likelihood
        mask for this call, and a recording chain records the log-probabilities with the predictor terms of the known elements left
        out -- the conditioned chain's trajectory likelihood up to a constant of the weights.  The states are those of the same call
        without the keyword, bit for bit.  None (the default): the record of the unconditioned proposal, as above.

        `resample` = (r, j) (with a condition): RePaint's resampling jumps.  At every jump-off level 1, 1 + j, 1 + 2 j, ... the
        whole state is re-noised j levels forward and denoised again, r visits in all, every repetition under a seed of its own
        (resampling.visit_seed); (1, j) is the plain conditioned chain, bit for bit.  The chain's handles carry (r, j) and the jump table
        for this call, like the condition.  ValueError before any device work: no condition, record=True, `noise`, `likelihood`,
        t_stop != 0, r < 1, j < 1, or no jump-off level (1 + j > t_start).

        `guidance` = guidance.Guidance(values, factor) (a property-conditioned module): the chain runs under the crystals' property
        values, and with factor != 0 every network evaluation is two -- the conditional one and the null one, on a cached partner handle
        per chain -- and the step takes p_c + factor (p_c - p_u).  Attached to the chain's handles for this call and cleared afterwards,
        like a condition; each stream group gets its crystals' slice.  Without it a property-conditioned module samples under the null
        row.  ValueError before any device work: a module without a property part, an unknown property, record=True, `condition`,
        `likelihood`, `resample`, CSP mode.

        `steer` = steering.Steering(predictor, task, ...): predictor-steered sampling.  `batch` holds K-replicated atom counts
        (Steering.replicate); the chain is walked as segments between the steering levels, and at each level the noise-aware predictor
        scores the particles' states and each group of K is resampled on the device -- one chain on one stream, nothing read inside it.
        Returns (final, traj, info): info = dict(levels, times, ancestors [E][B], stats [E][3]) from one read at the end.  On a view the
        levels are step indices and the predictor is given their trained times.  ValueError by name before any device work: a predictor
        that is not noised or of another T / schedule, atom counts that are not K-replicated, streams > 1, `record`, `noise`,
        `condition`, `likelihood`, `resample`, `guidance`, CSP mode.

        `classifier` = classifier.ClassifierGuidance(predictor, task, ...): classifier guidance from the noise-aware predictor's
        input gradient.  Every step t -> t - 1 of the guided window is the gradient at x_t (at the trained time of t on a view), one
        single-step segment, and the shift of the new state by scale * Sigma_t * gradient -- one chain on one stream, nothing read inside
        it.  Returns (final, traj, info): info = dict(levels, times, out [E][B]) from one read at the end.  ValueError by name before any
        device work: a predictor that is not noised, of another T / schedule or knn-style, streams > 1, `record`, `noise`, `condition`,
        `likelihood`, `resample`, `guidance`, `steer`, CSP mode, a property-conditioned prior.

        `symmetry` = symmetry_constraint.SymmetryConstraint for the crystals of `batch` (it may BE `batch`): the state is projected
        onto each crystal's group -- coordinates pulled back from the orbit representatives, the cell's metric averaged over the rotation
        parts, the type rows shared inside an orbit -- at the start and after the predictor of every step, behind any condition; the
        corrector is left alone.  Every state of the chain carries the group to float32 rounding.  The constraint is attached to the chain's
        batch handles for this call and cleared afterwards, each stream group its crystals' slice.  With `condition` as well: a condition
        on atom types alone, whose known types agree inside every orbit (checked on the host).  Returns (final, traj, info): info =
        dict(cell_failures [B]), the crystals' counts of cell projections skipped for a non-finite or non-positive metric, from one read at
        the end.  ValueError by name before any device work: `record`, `noise`, `likelihood`, `resample`, `guidance`, `steer`,
        `classifier`, CSP mode, atom counts that are not the batch's.
        """
        if symmetry is not None:
            for name, v in (("record=True", record), ("teacher-forced noise", noise is not None), ("likelihood", likelihood is not None),
                            ("resample", resample is not None), ("guidance", guidance is not None), ("steer", steer is not None),
                            ("classifier", classifier is not None), ("CSP mode", self.keep_lattice or self.keep_coords)):
                if v:
                    raise ValueError(f"sample: symmetry together with {name} is not supported -- a projected state has no likelihood under "
                                     "the recorded proposal, and the projection moves what the other keyword holds fixed (DESIGN 57)")
            counts = batch.num_atoms_list if isinstance(batch, CrystalBatch) else [int(v) for v in batch.num_atoms.tolist()]
            if [int(v) for v in symmetry.num_atoms.tolist()] != counts:
                raise ValueError("sample: the symmetry constraint's atom counts are not the batch's")
            if condition is not None:
                symmetry.check_condition(condition, "sample")
        if classifier is not None:
            from . import classifier as _classifier
            _classifier.check_call(self, classifier, streams=streams, record=record, noise=noise, condition=condition, likelihood=likelihood,
                                   resample=resample, guidance=guidance, steer=steer)
            if self.__dict__.get("_knn_pending"):
                self.check_graph()
            return _classifier.run_chain(self, batch, classifier, step_lr, seed, init, t_start, t_stop, node_offset, graph_offset)
        if steer is not None:
            from . import steering
            steering.check_call(self, steer, streams=streams, record=record, noise=noise, condition=condition, likelihood=likelihood,
                                resample=resample, guidance=guidance)
            steer.check_counts(batch.num_atoms_list if isinstance(batch, CrystalBatch) else batch.num_atoms)
            if self.__dict__.get("_knn_pending"):
                self.check_graph()
            return steering.run_chain(self, batch, steer, step_lr, seed, init, t_start, t_stop, node_offset, graph_offset)
        from .conditioning import check_likelihood
        from .resampling import check_chain
        gd = None
        if guidance is not None:
            from .guidance import module_condition
            module_condition(self, "sample(guidance=)")
            for name, v in (("record=True", record), ("a condition", condition is not None), ("likelihood", likelihood is not None),
                            ("resample", resample is not None), ("CSP mode", self.keep_lattice or self.keep_coords)):
                if v:
                    raise ValueError(f"sample: guidance together with {name} is not supported")
            gd = (guidance,) + guidance.arrays((self.base if self.base is not None else self).normalizer, len(batch.num_atoms))
        rj = None if resample is None else check_chain("sample", resample, self.beta_scheduler.timesteps, t_start, t_stop, condition, record,
                                                       noise, likelihood)
        lik = check_likelihood("sample", likelihood, condition)
        if condition is not None and [int(v) for v in condition.num_atoms.tolist()] != [int(v) for v in batch.num_atoms.tolist()]:
            raise ValueError("sample: the condition's atom counts are not the batch's")
        if self.__dict__.get("_knn_pending"):
            self.check_graph()   # (the verdict of the previous call's chains: by now they have long finished)
        sym = None if symmetry is None else (symmetry, [])   # (the constraint, the sink of its handles' failure counts)

        def result(final, traj):   # with a constraint: (final, traj, info)
            if sym is None:
                return final, traj
            import numpy as np
            return final, traj, dict(cell_failures=np.concatenate(sym[1]) if sym[1] else np.zeros(0, np.int64))
        if isinstance(batch, CrystalBatch):
            return result(*self._sample_one(batch, step_lr, seed, noise, init, record, t_start, t_stop, node_offset, graph_offset, rec_sink=rec_sink,
                                            condition=condition, likelihood=lik, resample=rj, guidance=gd, symmetry=sym))
        if (self.keep_lattice or self.keep_coords) and init is None and condition is None:
            # CSP mode (diffusion.py:283-287): the known part of the structure replaces the drawn initial state and is never moved
            cb0 = self.crystal_batch(batch, node_offset, graph_offset)
            dev = self.device
            x0, l0, a0 = (torch.empty(cb0.num_nodes, 3, device=dev), torch.empty(cb0.num_graphs, 3, 3, device=dev),
                          torch.empty(cb0.num_nodes, MAX_ATOMIC_NUM, device=dev))
            _lib.check(_lib.load().mi_sampler_init_state(cb0._h, seed, self.beta_scheduler.timesteps, _ptr(a0), _ptr(x0), _ptr(l0), _stream()))
            if self.keep_coords:
                x0 = batch.frac_coords.to(dev, torch.float32)
            if self.keep_lattice:
                from .data import lattice_params_to_matrix
                l0 = lattice_params_to_matrix(batch.lengths.to(dev, torch.float32), batch.angles.to(dev, torch.float32))
            init = (x0, l0, a0)
        na = [int(v) for v in batch.num_atoms.tolist()]
        if streams is None:
            e_total = sum(v * v for v in na)
            # measured: 2 chains +8 % at E = 26k (192 mp_20-sized crystals); at E = 102k 1/2/3/4/5 chains give
            # 24.3 / 25.8 / 26.7 / 27.4 / 22.8 structures/s (the runtime has four hardware queues)
            streams = 4 if e_total >= 98304 else 3 if e_total >= 49152 else 2 if e_total >= 16384 else 1
        streams = max(1, min(int(streams), len(na)))
        if streams == 1:
            return result(*self._sample_one(batch, step_lr, seed, noise, init, record, t_start, t_stop, node_offset, graph_offset, rec_sink=rec_sink,
                                            condition=condition, likelihood=lik, resample=rj, guidance=gd, symmetry=sym))
        key = ("split", streams, tuple(na))
        parts = getattr(batch, "_mi_split", {}).get(key)
        if parts is None:  # contiguous crystal groups, cached on the batch object like its CrystalBatch
            cuts = [len(na) * k // streams for k in range(streams + 1)]
            parts = [_Counts(na[cuts[k]:cuts[k + 1]]) for k in range(streams)]
            try:
                batch._mi_split = {key: parts}
            except AttributeError:
                pass
        g0 = [0]
        n0 = [0]
        for p_ in parts:
            g0.append(g0[-1] + len(p_.num_atoms))
            n0.append(n0[-1] + int(p_.num_atoms.sum()))
        self.decoder.sync()
        self._coefficients(step_lr)
        cur = torch.cuda.current_stream()
        # ONE state for the whole batch, allocated (and, with `init`, copied) here on the caller's stream; every chain works in place on ITS rows
        # of it.  (Each chain used to clone its slices on its own thread -- twelve small torch calls contending for the interpreter lock at the
        # head of every call, 70-150 us apart on the GPU timeline -- and the call ended with five torch.cat launches: profiles/r5_window_steps.log.)
        dev = self.device
        n_tot, b_tot = n0[-1], g0[-1]
        if init is not None:
            state = tuple(v.to(dev, torch.float32).contiguous().clone() for v in init)
        else:
            state = (torch.empty(n_tot, 3, device=dev), torch.empty(b_tot, 3, 3, device=dev), torch.empty(n_tot, MAX_ATOMIC_NUM, device=dev))
        ready = cur.record_event()
        sinks = [[] for _ in parts] if rec_sink is not None else [None] * len(parts)
        # long-lived worker threads, one per stream (streams.ChainWorkers): a call hands each its chain and waits -- no thread start per call
        from .streams import ChainWorkers
        workers = ChainWorkers.get(streams, self.device)

        # (starting chain k later by k x 150 ... 1 200 us was measured and costs the delay: DESIGN 19.7, profiles/r5_chain_stagger.log)
        def run(k, stream):
            stream.wait_event(ready)
            own = (state[0][n0[k]:n0[k + 1]], state[1][g0[k]:g0[k + 1]], state[2][n0[k]:n0[k + 1]])   # (contiguous row ranges: views, no copy)
            nz = None if noise is None else {"corr_x": noise["corr_x"][:, n0[k]:n0[k + 1]], "pred_x": noise["pred_x"][:, n0[k]:n0[k + 1]],
                                             "pred_t": noise["pred_t"][:, n0[k]:n0[k + 1]], "pred_l": noise["pred_l"][:, g0[k]:g0[k + 1]]}
            r = self._sample_one(parts[k], step_lr, seed, nz, None, record, t_start, t_stop, node_offset + n0[k], graph_offset + g0[k],
                                 inplace=own, drawn=init is not None, rec_sink=sinks[k])
            cur.wait_event(stream.record_event())
            return r

        # a condition is attached here, to every group's handle before the first chain is enqueued (the blocking copies do not wait between
        # the chains), and cleared when all of them are: each group gets its crystals' slice
        conds = [] if condition is None else [(self.crystal_batch(parts[k], node_offset + n0[k], graph_offset + g0[k]), condition.slice(g0[k], g0[k + 1]))
                                              for k in range(streams)]
        # ... and so is guidance: every group's handle gets its crystals' rows and a partner handle of its own
        guided = [] if gd is None else [(self.crystal_batch(parts[k], node_offset + n0[k], graph_offset + g0[k]), (node_offset + n0[k], graph_offset + g0[k]),
                                         gd[1][g0[k]:g0[k + 1]], gd[2][g0[k]:g0[k + 1]]) for k in range(streams)]
        # ... and so is a symmetry constraint, inside the condition's scope
        syms = [] if sym is None else [(self.crystal_batch(parts[k], node_offset + n0[k], graph_offset + g0[k]), sym[0].slice(g0[k], g0[k + 1]))
                                       for k in range(streams)]
        with self._conditioned(conds, likelihood=lik, resample=rj), self._guided(guided, gd), self._symmetric(syms, None if sym is None else sym[1]):
            out = workers.run(run, streams)
        if rec_sink is not None:
            for k, sk in enumerate(sinks):
                for _, _, bufs in sk:
                    for v in bufs.values():
                        v.record_stream(cur)   # (allocated on the group stream, consumed on the caller's)
                rec_sink.extend((g0[k] + g, n0[k] + n, bufs) for g, n, bufs in sk)

        def merge(ds):
            m = {}
            for d in ds:  # the parts were allocated on the group streams and are consumed on the caller's stream
                for v in d.values():
                    if torch.is_tensor(v) and v.is_cuda:
                        v.record_stream(cur)
            for name in ds[0]:
                if name == "batch_idx":
                    m[name] = torch.cat([d[name] + g0[k] for k, d in enumerate(ds)])
                else:
                    m[name] = torch.cat([d[name] for d in ds])
            return m

        def final_state():   # the chains' final states ARE the rows of `state`: nothing to concatenate
            idx = getattr(batch, "_mi_batch_idx", None)
            if idx is None or idx[0] != key:
                idx = (key, torch.cat([o[0]["batch_idx"] + g0[k] for k, o in enumerate(out)]), torch.cat([o[0]["num_atoms"] for o in out]))
                try:
                    batch._mi_batch_idx = idx
                except AttributeError:
                    pass
            return dict(atom_types=state[2], frac_coords=state[0], lattices=state[1], num_atoms=idx[2], batch_idx=idx[1])
        traj = {t: (final_state() if t == t_stop else merge([o[1][t] for o in out])) for t in out[0][1]}
        return result(traj[t_stop], traj)

    def check_graph(self):
        """knn edge style: wait for the chains enqueued by `sample` and raise (MI_ECAPACITY, as a RuntimeError) if a neighbour list built inside one of them
        exceeded its capacity -- the results of that chain are invalid.  Called by `sample` for the chains of EARLIER calls, by DiffCSPSampler.generate before
        it unpacks a batch, and by any caller about to read a chain's results.  A no-op for the fc edge style."""
        pending, self.__dict__["_knn_pending"] = self.__dict__.get("_knn_pending", []), []
        lib = _lib.load()
        for cb, stream in pending:
            rc = lib.mi_knn_graph_status(cb._h, C.c_void_p(stream.cuda_stream))
            cb.num_edges = int(lib.mi_batch_num_edges(cb._h))   # (the chain's last list, now that the host has seen its count; none behind a capacity error)
            _lib.check(rc, "mi_knn_graph_status")

    @contextlib.contextmanager
    def _conditioned(self, pairs, condition=True, likelihood=False, resample=None):
        """Attach each (batch handle, Condition) of `pairs` for the duration of the block and clear the handles afterwards, whatever happens
        inside: the cached handles of `crystal_batch` must not carry a condition into a later call.  The device is drained once first --
        an earlier chain of a cached handle may still be reading the arrays the attach overwrites.  `condition`: the condition itself
        (values and level table); `likelihood`: its masks as the handle's likelihood mask; either or both.  `resample`: (r, j), attached
        with this module's jump table alongside the condition."""
        if not pairs:
            yield
            return
        from . import resampling
        from .conditioning import Condition
        torch.cuda.synchronize(self.device)
        try:
            jumps = None if resample is None else resampling.jump_table(self, resample[1])
            for cb, c in pairs:
                if condition:
                    c.attach(self, cb)
                if likelihood:
                    c.attach_likelihood(self, cb)
                if resample is not None:
                    resampling.attach(self, cb, resample[0], resample[1], table=jumps)
            yield
        finally:
            for cb, _ in pairs:
                if condition:
                    Condition.clear(cb)
                if likelihood:
                    Condition.clear_likelihood(cb)
                if resample is not None:
                    resampling.clear(cb)

    @contextlib.contextmanager
    def _symmetric(self, pairs, sink):
        """Attach each (batch handle, SymmetryConstraint) of `pairs` for the duration of the block and clear the handles afterwards, whatever
        happens inside (_conditioned's contract: one drain of the device first).  Behind the block the device is drained once more and the
        handles' failure counters are read into `sink`, in the order of `pairs`."""
        if not pairs:
            yield
            return
        from . import symmetry_constraint as SC
        torch.cuda.synchronize(self.device)
        try:
            for cb, c in pairs:
                c.attach(cb)
            yield
            sink.extend(SC.failures(cb) for cb, _ in pairs)
        finally:
            for cb, _ in pairs:
                SC.SymmetryConstraint.clear(cb)

    @contextlib.contextmanager
    def _guided(self, handles, gd):
        """Attach guidance to each (batch handle, (node offset, graph offset), yhat rows, have rows) of `handles` for the duration of the block
        and clear the handles afterwards, whatever happens inside (_conditioned's contract: one drain of the device first).  gd =
        (Guidance, yhat, have) of the call.  With factor != 0 each handle gets a partner handle of its atom counts and offsets for the null
        evaluation, created on first use and kept on the handle."""
        if not handles:
            yield
            return
        import numpy as np
        from . import guidance as G
        torch.cuda.synchronize(self.device)
        try:
            for cb, off, yhat, have in handles:
                partner = None
                if gd[0].factor != 0.0:
                    partner = cb.__dict__.get("_mi_partner")
                    if partner is None:
                        partner = cb._mi_partner = self.make_batch(cb.num_atoms_list, int(off[0]), int(off[1]))
                G.attach(cb, partner, np.ascontiguousarray(yhat), np.ascontiguousarray(have), self.condition["num_freqs"], gd[0].factor)
            yield
        finally:
            for cb, *_ in handles:
                G.clear(cb)

    def _sample_one(self, batch, step_lr, seed, noise, init, record, t_start, t_stop, node_offset, graph_offset, inplace=None, drawn=False,
                    rec_sink=None, condition=None, likelihood=False, resample=None, guidance=None, symmetry=None):
        """One chain over one CrystalBatch on the current stream.

        Returns (traj[t_stop], traj) like the reference.  `traj` holds every step only when
        record=True (the reference keeps all T+1 states alive on the device); otherwise it
        holds the final state.  Noise comes from the library's counter-based Philox stream
        keyed by `seed` unless `noise` supplies per-step arrays (dict with corr_x/pred_l/
        pred_t/pred_x: [T+1, ...] tensors) and `init` the initial state (x_T, l_T, t_T).
        """
        lib = _lib.load()
        dev = self.device
        T = self.beta_scheduler.timesteps
        t_start = T if t_start is None else t_start
        cb = batch if isinstance(batch, CrystalBatch) else self.crystal_batch(batch, node_offset, graph_offset)
        B, N = cb.num_graphs, cb.num_nodes
        self.decoder.sync()
        if inplace is not None:   # (a chain of a split batch: its rows of the caller's state, updated in place; `drawn`: they already hold the initial state)
            x, l, a = inplace
            assert x.is_contiguous() and l.is_contiguous() and a.is_contiguous() and x.shape[0] == N and l.shape[0] == B
            if not drawn:
                _lib.check(lib.mi_sampler_init_state(cb._h, seed, T, _ptr(a), _ptr(x), _ptr(l), _stream()), "mi_sampler_init_state")
        elif init is None:
            x = torch.empty(N, 3, device=dev)
            l = torch.empty(B, 3, 3, device=dev)
            a = torch.empty(N, MAX_ATOMIC_NUM, device=dev)
            _lib.check(lib.mi_sampler_init_state(cb._h, seed, T, _ptr(a), _ptr(x), _ptr(l), _stream()), "mi_sampler_init_state")
        else:
            x, l, a = (v.to(dev, torch.float32).contiguous().clone() for v in init)
        # (traj[T]['frac_coords'] = x_T % 1, diffusion.py:289: mi_sampler_run wraps the coordinates in place before its first step -- no torch
        #  arithmetic on a chain's stream)
        coef = self._coefficients(step_lr)
        _lib.check(lib.mi_sampler_set_keep(cb._h, int(self.keep_lattice), int(self.keep_coords)))
        nz = None
        if noise is not None:
            keep = {k: noise[k].to(dev, torch.float32).contiguous() for k in ("corr_x", "pred_l", "pred_t", "pred_x")}
            nz = _lib.SamplerNoise(*(keep[k].data_ptr() for k in ("corr_x", "pred_l", "pred_t", "pred_x")))
        rec, rec_t = None, None
        if record:
            z = lambda *s: torch.zeros(*s, device=dev)
            rec_t = dict(atom_types=z(T + 1, N, MAX_ATOMIC_NUM), frac_coords=z(T + 1, N, 3), lattices=z(T + 1, B, 3, 3),
                         frac_coords_mid=z(T + 1, N, 3), log_prob_l=z(T + 1, B), log_prob_t=z(T + 1, B), log_prob_x=z(T + 1, B))
            rec = _lib.SamplerRecord(*(rec_t[k].data_ptr() for k in ("atom_types", "frac_coords", "lattices", "frac_coords_mid",
                                                                     "log_prob_l", "log_prob_t", "log_prob_x")))
        with self._conditioned([] if condition is None else [(cb, condition)], likelihood=likelihood, resample=resample), \
                self._guided([] if guidance is None else [(cb, (node_offset, graph_offset), guidance[1], guidance[2])], guidance), \
                self._symmetric([] if symmetry is None else [(cb, symmetry[0])], None if symmetry is None else symmetry[1]):
            _lib.check(lib.mi_sampler_run(self.decoder._h, cb._h, coef.numpy().ctypes.data_as(C.POINTER(C.c_float)), T, t_start, t_stop,
                                          _ptr(self.time_embedding.freqs), seed, C.byref(nz) if nz is not None else None,
                                          C.byref(rec) if rec is not None else None, _ptr(a), _ptr(x), _ptr(l), _stream()),
                       "mi_sampler_run")
        if cb.edge_style == "knn":
            # the chain rebuilt its periodic neighbour list in every evaluation WITHOUT a host round trip (the reference synchronises per evaluation:
            # cspnet.py:243-257); a list over capacity could not raise inside the enqueued chain -- its verdict waits on the batch handle for check_graph()
            self.__dict__.setdefault("_knn_pending", []).append((cb, torch.cuda.current_stream()))
        final = dict(atom_types=a, frac_coords=x, lattices=l, num_atoms=cb.num_atoms, batch_idx=cb.batch)
        traj = {t_stop: final}
        if record and rec_sink is not None:
            rec_sink.append((0, 0, rec_t))
        if record:
            for t in range(t_start, t_stop - 1, -1):
                d = dict(atom_types=rec_t["atom_types"][t], frac_coords=rec_t["frac_coords"][t], lattices=rec_t["lattices"][t],
                         num_atoms=cb.num_atoms, batch_idx=cb.batch)
                if t > max(t_stop, 1):
                    d.update(log_prob_l=rec_t["log_prob_l"][t], log_prob_t=rec_t["log_prob_t"][t],
                             log_prob_x=rec_t["log_prob_x"][t], frac_coords_mid=rec_t["frac_coords_mid"][t])
                traj[t] = d
        return final, traj

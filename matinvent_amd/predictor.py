"""Property predictor: the CSPNet trunk with a scalar head, trained on labelled crystals and used as a reward.

The reference's CSPNet(pred_scalar=True) (models/diffcsp/cspnet.py:145-147, 281-284) pools the final node features per crystal with a mean
and applies scalar_out = nn.Linear(hidden_dim, 1).  Here the head has P >= 1 outputs (P = 1: the reference), one per property name:

    out[b][p] = bias[p] + sum_f mean_i(hf_i)[f] W[p][f]                                    (normalised units)
    loss      = sum_p (1 / P) sum_{b: target present} l(out - yhat) / count[p]             l = e^2 ("mse") or |e| ("l1")

Every call is one entry of include/matinvent_hip_scalar.h: the clean inputs at time 0, the trunk, the head, the loss with its statistics
and -- training -- the backward, enqueued with no host synchronisation.  The model keeps ONE flat vector [trunk theta | W | bias]; the
trunk's parameter vector is a view of its head, so FusedAdam's clipping, guard and average work on it as on any flat parameter.
"""
import contextlib
import ctypes as C
import logging
import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import config as CFG
from .guidance import PropertyNormalizer

LOSS_KINDS = {"mse": _lib.SCALAR_LOSS_MSE, "l1": _lib.SCALAR_LOSS_L1}
HPARAMS_FILE, WEIGHTS_FILE = "hparams.yaml", "last.ckpt"
HPARAM_KEYS = ("names", "hidden_dim", "num_layers", "time_dim", "num_freqs", "ln", "edge_style")


def stats_len(P):
    """mi_scalar_micro_step's stats: [0] loss, then per property sum e^2, sum |e|, present targets."""
    return 1 + 3 * int(P)


def _names(names):
    names = [names] if isinstance(names, str) else [str(n) for n in (names or [])]
    if not names or len(set(names)) != len(names):
        raise ValueError(f"PropertyPredictor: the property names {names} must be distinct and at least one")
    return names


class PropertyPredictor(nn.Module):
    """The trunk (a CSPNet of the DiffCSPModule configuration, whose three heads are never evaluated here), the head and the normaliser.
    names: the properties, one head row each.  seed: the initial weights are drawn under it (None: torch's global generator).
    latent_dim > 0 (a property-conditioned trunk) is refused: ValueError, before any device work."""

    def __init__(self, names, hidden_dim=128, num_layers=4, time_dim=256, num_freqs=10, ln=True, edge_style="fc", normalizer=None, device=None,
                 seed=None, latent_dim=0):
        super().__init__()
        self.names = _names(names)
        if int(latent_dim) != 0:
            raise ValueError(f"PropertyPredictor: latent_dim = {latent_dim}: a latent (property-conditioned) net has no predictor form; "
                             "the trunk's embedding input is the time embedding alone")
        if normalizer is not None and list(normalizer.names) != self.names:
            raise ValueError(f"PropertyPredictor: the normaliser's names {list(normalizer.names)} differ from the model's {self.names}")
        from .cspnet import CSPNet
        from .schedules import time_embedding_freqs
        self.hparams = dict(names=list(self.names), hidden_dim=int(hidden_dim), num_layers=int(num_layers), time_dim=int(time_dim),
                            num_freqs=int(num_freqs), ln=bool(ln), edge_style=str(edge_style))
        with contextlib.ExitStack() as st:
            if seed is not None:
                st.enter_context(torch.random.fork_rng(devices=[]))
                torch.manual_seed(int(seed))
            trunk = CSPNet(hidden_dim=hidden_dim, latent_dim=time_dim, num_layers=num_layers, num_freqs=num_freqs, edge_style=edge_style, ln=ln,
                           smooth=True, pred_type=True, device=device)
            H, P = int(hidden_dim), len(self.names)
            head = nn.Linear(H, P)   # (nn.Linear's default init, drawn behind the trunk's: the reference's construction order)
        self.__dict__["trunk"] = trunk   # (not a sub-module: its parameter is a view of `flat`, the one parameter of this module)
        self.n_trunk = trunk.theta.numel()
        dev = trunk.theta.device
        flat = torch.cat([trunk.theta.data.reshape(-1), head.weight.data.reshape(-1).to(dev), head.bias.data.reshape(-1).to(dev)])
        self.flat = nn.Parameter(flat.contiguous())
        self.register_buffer("time_freqs", time_embedding_freqs(time_dim).to(dev, torch.float32).contiguous(), persistent=False)
        self.normalizer = normalizer if normalizer is not None else PropertyNormalizer(self.names)
        self._tie()

    # ---- the flat vector ---------------------------------------------------------------------------
    def _tie(self):
        """The trunk's theta becomes the head of `flat` (same memory), and `flat` names this module as the owner an optimizer tells about
        an in-place update."""
        t = nn.Parameter(self.flat.data[:self.n_trunk], requires_grad=False)
        t._mi_owner = self.trunk
        self.trunk.theta = t
        self.trunk.mark_dirty()
        self.flat._mi_owner = self

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._tie()
        return r

    def mark_dirty(self):
        self.trunk.mark_dirty()

    @property
    def P(self):
        return len(self.names)

    @property
    def hidden_dim(self):
        return self.trunk.hidden_dim

    @property
    def noised(self):
        """None: a predictor of clean inputs at time 0 (every predictor saved before DESIGN 43).  A dict (noised_spec: T and the schedules'
        defining parameters): trained by fit_predictor(diffusion=) on forward-noised inputs at drawn times 0..T of that schedule -- what
        steering.Steering and every other caller that needs a noise-aware predictor ask for by name (require_noised)."""
        return self.hparams.get("noised")

    @property
    def device(self):
        return self.flat.device

    def head_slices(self, v=None):
        """(trunk, W [P H], bias [P]) views of a vector laid out like `flat` (default: flat's data)."""
        v = self.flat.data if v is None else v
        n, k = self.n_trunk, self.P * self.hidden_dim
        return v[:n], v[n:n + k], v[n + k:]

    def set_normalizer(self, nm):
        if list(nm.names) != self.names:
            raise ValueError(f"PropertyPredictor: the normaliser's names {list(nm.names)} differ from the model's {self.names}")
        self.normalizer = nm

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        """The reference's names: scalar_out.weight [P, H], scalar_out.bias [P], then the trunk's tensors."""
        from collections import OrderedDict
        out = destination if destination is not None else OrderedDict()
        _, W, b = self.head_slices()
        out[prefix + "scalar_out.weight"] = W.detach().clone().view(self.P, self.hidden_dim)
        out[prefix + "scalar_out.bias"] = b.detach().clone()
        return self.trunk.state_dict(destination=out, prefix=prefix)

    def load_state_dict(self, state_dict, strict=True):
        _, W, b = self.head_slices()
        missing = [k for k in ("scalar_out.weight", "scalar_out.bias") if k not in state_dict]
        with torch.no_grad():
            if "scalar_out.weight" in state_dict:
                W.copy_(state_dict["scalar_out.weight"].reshape(-1))
            if "scalar_out.bias" in state_dict:
                b.copy_(state_dict["scalar_out.bias"].reshape(-1))
        errs = []
        self.trunk._load_from_state_dict(state_dict, "", {}, strict, missing, [], errs)
        if strict and missing:
            raise KeyError(f"PropertyPredictor.load_state_dict: missing {missing}")
        self.trunk.mark_dirty()
        return missing

    def make_batch(self, num_atoms, node_offset=0, graph_offset=0, pool=None):
        return self.trunk.make_batch(num_atoms, node_offset, graph_offset, pool=pool)

    def predict(self, records_or_batch, batch_size=64, pool=None):
        return predict(self, records_or_batch, batch_size=batch_size, pool=pool)


# ---- records --------------------------------------------------------------------------------------------
def _record_fields(r):
    """(atomic numbers [n] int64, frac [n, 3] float32, lengths [3], angles [3]) of a CrystalData, a SimpleStructure, a read_extxyz frame or
    a pymatgen Structure; raises for anything that is not a crystal."""
    if hasattr(r, "atom_types"):
        z = np.asarray(r.atom_types.cpu() if torch.is_tensor(r.atom_types) else r.atom_types).reshape(-1)
        tn = lambda x: np.asarray(x.cpu() if torch.is_tensor(x) else x, dtype=np.float64)
        return z.astype(np.int64), tn(r.frac_coords).reshape(-1, 3), tn(r.lengths).reshape(3), tn(r.angles).reshape(3)
    if hasattr(r, "lattice") and hasattr(r.lattice, "abc"):   # pymatgen
        return (np.asarray(r.atomic_numbers, dtype=np.int64), np.asarray(r.frac_coords, dtype=np.float64).reshape(-1, 3),
                np.asarray(r.lattice.abc, dtype=np.float64), np.asarray(r.lattice.angles, dtype=np.float64))
    return (np.asarray([int(z) for z in r.species], dtype=np.int64), np.asarray(r.frac_coords, dtype=np.float64).reshape(-1, 3),
            np.asarray(r.lengths, dtype=np.float64).reshape(3), np.asarray(r.angles, dtype=np.float64).reshape(3))


def _valid_fields(r):
    """_record_fields, or None for a record the network cannot take: no atom, an atomic number outside 1..100, a non-finite value."""
    try:
        z, x, le, an = _record_fields(r)
    except Exception:
        return None
    if z.size < 1 or x.shape[0] != z.size or z.min() < 1 or z.max() > 100:
        return None
    if not (np.isfinite(x).all() and np.isfinite(le).all() and np.isfinite(an).all()):
        return None
    return z, x, le, an


class _Arrays:
    """The collated arrays of a list of _record_fields tuples (what train_step reads of a CrystalBatchData)."""

    def __init__(self, fields):
        self.num_atoms = [int(f[0].size) for f in fields]
        self.atom_types = torch.from_numpy(np.concatenate([f[0] for f in fields])) if fields else torch.zeros(0, dtype=torch.long)
        self.frac_coords = torch.from_numpy(np.concatenate([f[1] for f in fields]).astype(np.float32)) if fields else torch.zeros(0, 3)
        self.lengths = torch.from_numpy(np.stack([f[2] for f in fields]).astype(np.float32)) if fields else torch.zeros(0, 3)
        self.angles = torch.from_numpy(np.stack([f[3] for f in fields]).astype(np.float32)) if fields else torch.zeros(0, 3)


def _counts(batch):
    na = batch.num_atoms
    return [int(v) for v in (na.tolist() if torch.is_tensor(na) else na)]


def _times(times, B, dev):
    tm = torch.as_tensor(times).reshape(-1).to(dev, torch.int32).contiguous()
    if tm.numel() != B:
        raise ValueError(f"times holds {tm.numel()} values for {B} crystals")
    return tm


# ---- one call ---------------------------------------------------------------------------------------------
def train_step(model, batch, y=None, grad=None, stats=None, count_global=None, accum_steps=1, loss="mse", forward_only=False, out=None,
               pool=None, offsets=(0, 0), yhat=None, have=None, handle=None, t_all=0, times=None):
    """One micro-step on the current stream (mi_scalar_micro_step): `batch` (num_atoms, lengths, angles, frac_coords, atom_types) against
    the raw targets y [B][P] (NaN: missing), normalised by the model's normaliser -- or yhat / have, already normalised.  Accumulates (+=)
    into `grad` (laid out like model.flat; default flat.grad, allocated when absent) and `stats` (stats_len(P) device floats; returned).
    count_global [P]: the present targets per property the loss is normalised by (default: this batch's own).  forward_only=True: no tape,
    no backward, `grad` untouched (the validation form).  out: [B][P] device floats for the normalised predictions, or None.
    handle: a CrystalBatch of these atom counts to run on (kept by the caller); None: a handle for this call only, from `pool` when given
    (nothing then waits for the device).  times [B] ints: the crystals' time steps of the time embedding (default: t_all for all; the
    predictor of this module is trained and used at time 0)."""
    if loss not in LOSS_KINDS:
        raise ValueError(f"train_step: loss = {loss!r}: it takes 'mse' or 'l1'")
    lib = _lib.load()
    from .cspnet import _ptr, _stream
    dev = model.device
    na = _counts(batch)
    B, P = len(na), model.P
    if yhat is None:
        if y is None:
            raise ValueError("train_step: no targets (y, or yhat and have)")
        ya = np.asarray(y.cpu() if torch.is_tensor(y) else y, dtype=np.float64)
        if ya.size != B * P:
            raise ValueError(f"train_step: y holds {ya.size} values for {B} crystals x {P} properties")
        yhat, have = model.normalizer.normalise(ya)
    yhat = np.ascontiguousarray(np.asarray(yhat, dtype=np.float32).reshape(B, P))
    have = np.ascontiguousarray(np.asarray(have, dtype=np.int32).reshape(B, P))
    cg = have.sum(axis=0) if count_global is None else np.asarray(count_global)
    cg = np.ascontiguousarray(cg.reshape(P), dtype=np.int32)
    if stats is None:
        stats = torch.zeros(stats_len(P), device=dev)
    if not forward_only and grad is None:
        if model.flat.grad is None:
            model.flat.grad = torch.zeros_like(model.flat)
        grad = model.flat.grad
    if B == 0:
        return stats
    f = lambda x: x.to(dev, torch.float32).contiguous()
    lengths, angles, frac0 = f(batch.lengths).view(-1, 3), f(batch.angles).view(-1, 3), f(batch.frac_coords)
    at = batch.atom_types.to(dev, torch.int32).contiguous()
    tm = None if times is None else _times(times, B, dev)
    up = (lambda a: torch.from_numpy(a).to(dev)) if pool is None else (lambda a: torch.from_numpy(a).pin_memory().to(dev, non_blocking=True))
    yhat_d, have_d, cg_d = up(yhat), up(have), up(cg)
    model.trunk.sync()
    _, W, bias = model.head_slices()
    g = (None, None, None) if forward_only else model.head_slices(grad)
    cb = handle if handle is not None else model.make_batch(na, int(offsets[0]), int(offsets[1]), pool=pool)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    try:
        _lib.check(lib.mi_scalar_micro_step(model.trunk._h, cb._h, _ptr(lengths), _ptr(angles), _ptr(frac0), _ptr(at), _ptr(model.time_freqs), _ptr(tm),
                                            int(t_all), _ptr(W), _ptr(bias), P, _ptr(yhat_d), _ptr(have_d), ip(have), _ptr(cg_d), ip(cg),
                                            int(accum_steps), LOSS_KINDS[loss], _ptr(g[0]), _ptr(g[1]), _ptr(g[2]), _ptr(stats), _ptr(out), _stream()),
                   "mi_scalar_micro_step")
    finally:
        if handle is None:
            if pool is None:   # (the handle's memory is freed here: the host waits for the micro-step; a pooled handle frees nothing)
                torch.cuda.current_stream().synchronize()
            cb.release()
    return stats


def forward(model, batch, handle=None, pool=None, t_all=0, times=None):
    """The normalised predictions [B][P] (device) of `batch` on the current stream: mi_scalar_forward.  times: as train_step's."""
    lib = _lib.load()
    from .cspnet import _ptr, _stream
    dev = model.device
    na = _counts(batch)
    B, P = len(na), model.P
    out = torch.empty(B, P, device=dev)
    if B == 0:
        return out
    f = lambda x: x.to(dev, torch.float32).contiguous()
    lengths, angles, frac0 = f(batch.lengths).view(-1, 3), f(batch.angles).view(-1, 3), f(batch.frac_coords)
    at = batch.atom_types.to(dev, torch.int32).contiguous()
    tm = None if times is None else _times(times, B, dev)
    model.trunk.sync()
    _, W, bias = model.head_slices()
    cb = handle if handle is not None else model.make_batch(na, pool=pool)
    try:
        _lib.check(lib.mi_scalar_forward(model.trunk._h, cb._h, _ptr(lengths), _ptr(angles), _ptr(frac0), _ptr(at), _ptr(model.time_freqs), _ptr(tm),
                                         int(t_all), _ptr(W), _ptr(bias), P, _ptr(out), _stream()), "mi_scalar_forward")
    finally:
        if handle is None:
            if pool is None:
                torch.cuda.current_stream().synchronize()
            cb.release()
    return out


# ---- the noise-aware predictor (include/matinvent_hip_steer.h) ------------------------------------------------------------------
_NOISED_TIME_TAG = 0x6E74696D   # (draw_noised_times' generator shares a key with no other)


def noised_spec(diffusion):
    """What a noise-aware predictor records of the diffusion module it was trained under: T and the scalar constructor arguments of the
    two schedulers (of the module of the trained grid: a respaced view gives its base's)."""
    base = diffusion.base if getattr(diffusion, "base", None) is not None else diffusion
    if hasattr(base, "collate") or not hasattr(base, "beta_scheduler"):
        raise ValueError("a noise-aware predictor is trained under a DiffCSPModule (the MatterGen-shaped module has no such schedule here)")
    scal = lambda d: {str(k): (v if isinstance(v, (bool, int, str)) else float(v)) for k, v in dict(d).items()
                      if not str(k).startswith("_") and isinstance(v, (bool, int, float, str))}
    return dict(T=int(base.beta_scheduler.timesteps), beta_scheduler=scal(base.hparams["beta_scheduler"]),
                sigma_scheduler=scal(base.hparams["sigma_scheduler"]))


def require_noised(model, where, diffusion=None):
    """ValueError by name unless `model` is a noise-aware predictor -- and, with `diffusion`, one of that module's T and schedule."""
    spec = getattr(model, "noised", None)
    if spec is None:
        raise ValueError(f"{where}: the predictor is not noised (PropertyPredictor.noised is None: it was trained on clean inputs at time 0; "
                         "train one with fit_predictor(..., diffusion=module))")
    if diffusion is not None:
        want = noised_spec(diffusion)
        if int(spec.get("T", -1)) != want["T"]:
            raise ValueError(f"{where}: the predictor was trained with T = {spec.get('T')}, the module has T = {want['T']}")
        if dict(spec) != want:
            raise ValueError(f"{where}: the predictor's schedule {dict(spec)} differs from the module's {want}")
    return spec


def draw_noised_times(B, T, epoch, step, seed):
    """[B] int32 times, uniform in 0..T (0: the clean row -- a predictor that steers a chain is also asked at its end), from a numpy
    Generator keyed by (seed, epoch, step)."""
    return np.random.default_rng([_NOISED_TIME_TAG, int(seed), int(epoch), int(step)]).integers(0, int(T) + 1, size=int(B)).astype(np.int32)


def train_step_noised(model, batch, times, diffusion, y=None, noise=None, grad=None, stats=None, count_global=None, accum_steps=1, loss="mse",
                      forward_only=False, out=None, pool=None, offsets=(0, 0), yhat=None, have=None, handle=None, seed=0, call_id=None):
    """train_step on FORWARD-NOISED inputs (mi_scalar_micro_step_noised): crystal c at times[c] in 0..T of `diffusion`'s schedule (its
    pretrain.schedule_table; a respaced view gives its base's), noised by Philox draws 7-9 at `call_id` (default: the model's running
    counter, advanced) under `seed`, indexed through `offsets` -- or by the injected noise = (rand_l [B][9], rand_x [N][3], rand_t [N][100]).
    Everything else is train_step's."""
    if loss not in LOSS_KINDS:
        raise ValueError(f"train_step_noised: loss = {loss!r}: it takes 'mse' or 'l1'")
    from .pretrain import schedule_table
    base = diffusion.base if getattr(diffusion, "base", None) is not None else diffusion
    noised_spec(base)
    T = int(base.beta_scheduler.timesteps)
    lib = _lib.load()
    from .cspnet import _ptr, _stream
    dev = model.device
    na = _counts(batch)
    B, P = len(na), model.P
    th = np.ascontiguousarray(np.asarray(times.cpu() if torch.is_tensor(times) else times), dtype=np.int32).reshape(-1)
    if th.shape[0] != B:
        raise ValueError(f"train_step_noised: {th.shape[0]} times for {B} crystals")
    if B and (int(th.min()) < 0 or int(th.max()) > T):
        raise ValueError(f"train_step_noised: times must lie in 0..{T} (got {int(th.min())}..{int(th.max())})")
    if yhat is None:
        if y is None:
            raise ValueError("train_step_noised: no targets (y, or yhat and have)")
        ya = np.asarray(y.cpu() if torch.is_tensor(y) else y, dtype=np.float64)
        if ya.size != B * P:
            raise ValueError(f"train_step_noised: y holds {ya.size} values for {B} crystals x {P} properties")
        yhat, have = model.normalizer.normalise(ya)
    yhat = np.ascontiguousarray(np.asarray(yhat, dtype=np.float32).reshape(B, P))
    have = np.ascontiguousarray(np.asarray(have, dtype=np.int32).reshape(B, P))
    cg = have.sum(axis=0) if count_global is None else np.asarray(count_global)
    cg = np.ascontiguousarray(cg.reshape(P), dtype=np.int32)
    if stats is None:
        stats = torch.zeros(stats_len(P), device=dev)
    if not forward_only and grad is None:
        if model.flat.grad is None:
            model.flat.grad = torch.zeros_like(model.flat)
        grad = model.flat.grad
    if call_id is None:
        model.__dict__["_noise_calls"] = model.__dict__.get("_noise_calls", 0) + 1
        call_id = model.__dict__["_noise_calls"]
    if B == 0:
        return stats
    f = lambda x: x.to(dev, torch.float32).contiguous()
    lengths, angles, frac0 = f(batch.lengths).view(-1, 3), f(batch.angles).view(-1, 3), f(batch.frac_coords)
    at = batch.atom_types.to(dev, torch.int32).contiguous()
    up = (lambda a: torch.from_numpy(a).to(dev)) if pool is None else (lambda a: torch.from_numpy(a).pin_memory().to(dev, non_blocking=True))
    yhat_d, have_d, cg_d, t_dev = up(yhat), up(have), up(cg), up(th)
    nz = (None, None, None) if noise is None else tuple(None if x is None else f(x) for x in noise)
    table = schedule_table(base).to(dev)
    model.trunk.sync()
    _, W, bias = model.head_slices()
    g = (None, None, None) if forward_only else model.head_slices(grad)
    cb = handle if handle is not None else model.make_batch(na, int(offsets[0]), int(offsets[1]), pool=pool)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    try:
        _lib.check(lib.mi_scalar_micro_step_noised(model.trunk._h, cb._h, _ptr(lengths), _ptr(angles), _ptr(frac0), _ptr(at), _ptr(model.time_freqs), ip(th),
                                                   _ptr(t_dev), _ptr(table), T, int(seed), int(call_id) & 0xFFFFFFFF, _ptr(nz[0]), _ptr(nz[1]), _ptr(nz[2]),
                                                   _ptr(W), _ptr(bias), P, _ptr(yhat_d), _ptr(have_d), ip(have), _ptr(cg_d), ip(cg), int(accum_steps),
                                                   LOSS_KINDS[loss], _ptr(g[0]), _ptr(g[1]), _ptr(g[2]), _ptr(stats), _ptr(out), _stream()),
                   "mi_scalar_micro_step_noised")
    finally:
        if handle is None:
            if pool is None:
                torch.cuda.current_stream().synchronize()
            cb.release()
    return stats


def forward_state(model, state, handle, t, out=None):
    """The normalised predictions [B][P] (device) of a chain STATE on the current stream (mi_scalar_forward_state): state = a dict with
    atom_types [N][100] float rows, frac_coords [N][3], lattices [B][3][3] (a chain's arrays, read where they are and left unchanged) or
    the tuple (frac_coords, lattices, atom_types) of sample(init=); handle: a batch handle of THIS model (model.make_batch) with the
    state's atom counts -- never the chain's; t: the trained time, one int for all or [B] ints.  No host synchronisation."""
    lib = _lib.load()
    from .cspnet import _ptr, _stream
    dev = model.device
    x, l, a = (state["frac_coords"], state["lattices"], state["atom_types"]) if isinstance(state, dict) else state
    B, N, P = handle.num_graphs, handle.num_nodes, model.P
    f = lambda v: v.to(dev, torch.float32).contiguous()
    x, l, a = f(x), f(l), f(a)
    if a.numel() != N * _lib.NUM_TYPES or x.numel() != N * 3 or l.numel() != B * 9:
        raise ValueError(f"forward_state: the state's shapes {tuple(a.shape)}, {tuple(x.shape)}, {tuple(l.shape)} are not the handle's {N} atoms in {B} crystals")
    tm, t_all = (None, int(t)) if isinstance(t, (int, np.integer)) else (_times(t, B, dev), 0)
    if out is None:
        out = torch.empty(B, P, device=dev)
    if B == 0:
        return out
    model.trunk.sync()
    _, W, bias = model.head_slices()
    _lib.check(lib.mi_scalar_forward_state(model.trunk._h, handle._h, _ptr(a), _ptr(x), _ptr(l), _ptr(model.time_freqs), _ptr(tm), t_all, _ptr(W),
                                           _ptr(bias), P, _ptr(out), _stream()), "mi_scalar_forward_state")
    return out


GUIDE_MODES = {"max": _lib.GUIDE_MODE_MAX, "min": _lib.GUIDE_MODE_MIN, "target": _lib.GUIDE_MODE_TARGET}


def guide_seed(model, out, task, mode="max", target=None, d_out=None):
    """d_out [B][P] (device) of log p(y | x_t) from the normalised predictions `out` (mi_guide_seed): column `task` = +1 ("max"), -1 ("min")
    or -(out - target_hat) ("target": the raw value aimed at, normalised here), every other column 0, a row whose prediction is not finite
    all zeros.  No host synchronisation."""
    from .cspnet import _ptr, _stream
    if task not in model.names:
        raise ValueError(f"guide_seed: task = {task!r} is not a property of the predictor ({model.names})")
    if mode not in GUIDE_MODES:
        raise ValueError(f"guide_seed: mode = {mode!r}: it takes 'max', 'min' or 'target'")
    if (mode == "target") != (target is not None):
        raise ValueError("guide_seed: target = goes with mode = 'target', and only with it")
    p = model.names.index(task)
    that = 0.0 if target is None else (float(target) - float(model.normalizer.mean[p])) / float(model.normalizer.std[p])
    B, P = out.shape
    if d_out is None:
        d_out = torch.empty(B, P, device=out.device)
    _lib.check(_lib.load().mi_guide_seed(_ptr(out), int(B), int(P), p, GUIDE_MODES[mode], that, _ptr(d_out), _stream()), "mi_guide_seed")
    return d_out


def input_gradient(model, state, handle, t, d_out=None, task=None, mode="max", target=None, types=True, bufs=None):
    """(out, g_frac, g_lat, g_types): the normalised predictions [B][P] of a chain STATE and, per crystal b, the gradient of
    sum_p d_out[b][p] out[b][p] with respect to its coordinates [N][3], lattice [B][3][3] and type rows [N][100] (mi_scalar_input_grad: the
    taped forward and the trunk's data-only backward; types = False: g_types is None and not computed).  d_out: [B][P] -- or None: the
    seed of guide_seed(task, mode, target) from the predictions of forward_state at the same state (one more inference forward).  state,
    handle and t are forward_state's; the state's arrays are left unchanged.  A noise-aware predictor only.  No host synchronisation."""
    require_noised(model, "input_gradient")
    lib = _lib.load()
    from .cspnet import _ptr, _stream
    dev = model.device
    x, l, a = (state["frac_coords"], state["lattices"], state["atom_types"]) if isinstance(state, dict) else state
    B, N, P = handle.num_graphs, handle.num_nodes, model.P
    f = lambda v: v.to(dev, torch.float32).contiguous()
    x, l, a = f(x), f(l), f(a)
    if a.numel() != N * _lib.NUM_TYPES or x.numel() != N * 3 or l.numel() != B * 9:
        raise ValueError(f"input_gradient: the state's shapes {tuple(a.shape)}, {tuple(x.shape)}, {tuple(l.shape)} are not the handle's {N} atoms in {B} crystals")
    if d_out is None:
        if task is None:
            raise ValueError("input_gradient: give d_out [B][P], or task (with mode / target) for the seed of guide_seed")
        d_out = guide_seed(model, forward_state(model, (x, l, a), handle, t), task, mode, target, d_out=None if bufs is None else bufs["d_out"])
    else:
        d_out = f(d_out)
        if tuple(d_out.shape) != (B, P):
            raise ValueError(f"input_gradient: d_out has shape {tuple(d_out.shape)}, not ({B}, {P})")
    tm, t_all = (None, int(t)) if isinstance(t, (int, np.integer)) else (_times(t, B, dev), 0)
    if bufs is None:
        bufs = dict(out=torch.empty(B, P, device=dev), g_frac=torch.empty(N, 3, device=dev), g_lat=torch.empty(B, 3, 3, device=dev),
                    g_types=torch.empty(N, _lib.NUM_TYPES, device=dev) if types else None)
    out, g_frac, g_lat, g_types = bufs["out"], bufs["g_frac"], bufs["g_lat"], bufs["g_types"] if types else None
    if B == 0:
        return out, g_frac, g_lat, g_types
    model.trunk.sync()
    _, W, bias = model.head_slices()
    _lib.check(lib.mi_scalar_input_grad(model.trunk._h, handle._h, _ptr(a), _ptr(x), _ptr(l), _ptr(model.time_freqs), _ptr(tm), t_all, _ptr(W), _ptr(bias),
                                        P, _ptr(d_out), _ptr(out), _ptr(g_types), _ptr(g_frac), _ptr(g_lat), _stream()), "mi_scalar_input_grad")
    return out, g_frac, g_lat, g_types


def predict(model, records_or_batch, batch_size=64, pool=None):
    """De-normalised predictions, np.ndarray [n][P] float64, of a list of records (CrystalData, structures, read_extxyz frames) or of a
    CrystalBatchData.  A crystal that cannot be evaluated -- no atoms, an atomic number outside 1..100, a non-finite value, an atom count
    the batch handle refuses -- is a row of NaN, never an exception for the others."""
    if int(batch_size) < 1:
        raise ValueError(f"predict: batch_size = {batch_size}: must be >= 1")
    P = model.P
    mean, std = np.asarray(model.normalizer.mean, dtype=np.float64), np.asarray(model.normalizer.std, dtype=np.float64)
    if hasattr(records_or_batch, "num_atoms") and hasattr(records_or_batch, "frac_coords") and not hasattr(records_or_batch, "properties"):
        b = records_or_batch   # a collated batch: cut back into records
        na = _counts(b)
        off = np.concatenate([[0], np.cumsum(na)])
        ten = lambda x: np.asarray(x.detach().cpu())
        z, x, le, an = ten(b.atom_types), ten(b.frac_coords), ten(b.lengths).reshape(-1, 3), ten(b.angles).reshape(-1, 3)
        from types import SimpleNamespace
        records = [SimpleNamespace(species=z[off[i]:off[i + 1]].tolist(), frac_coords=x[off[i]:off[i + 1]], lengths=le[i], angles=an[i])
                   for i in range(len(na))]
    else:
        records = list(records_or_batch)
    out = np.full((len(records), P), np.nan, dtype=np.float64)
    fields = [_valid_fields(r) for r in records]
    ok = [i for i, f in enumerate(fields) if f is not None]
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            pend = []   # (rows, device result): read once at the end
            for s in range(0, len(ok), int(batch_size)):
                rows = ok[s:s + int(batch_size)]
                try:
                    pend.append((rows, forward(model, _Arrays([fields[i] for i in rows]), pool=pool)))
                except _lib.MIError:
                    for i in rows:   # one crystal of the batch is refused: each on its own, the refused one stays NaN
                        try:
                            pend.append(([i], forward(model, _Arrays([fields[i]]), pool=pool)))
                        except _lib.MIError:
                            pass
            for rows, o in pend:
                out[rows] = o.double().cpu().numpy() * std + mean
    finally:
        model.train(was_training)
    return out


EVAL_CALL = 0   # the Philox call id of a noised evaluation (noised training counts from 1)


def _eval_enqueue(model, data_list, batch_size, acc, loss="mse", pool=None, diffusion=None, t=None, seed=0):
    """`evaluate` without the read-back: every mini-batch of the set in order, forward-only, normalised by the counts of the WHOLE set.
    diffusion: the noised form -- every crystal at time `t`, or (t None) at times drawn under (seed, epoch 0, mini-batch index): the same
    noised validation set every epoch."""
    from .data import CrystalBatchData
    from .pretrain import batch_plan
    yh, hv = model.normalizer(data_list)
    cg = hv.sum(axis=0)
    n0 = 0
    for step, idx in enumerate(batch_plan(len(data_list), batch_size, 0, 0, shuffle=False)):
        b = CrystalBatchData([data_list[i] for i in idx])
        if diffusion is None:
            train_step(model, b, yhat=yh[idx], have=hv[idx], stats=acc, count_global=cg, loss=loss, forward_only=True, pool=pool)
        else:
            T = noised_spec(diffusion)["T"]
            tm = np.full(len(idx), int(t), np.int32) if t is not None else draw_noised_times(len(idx), T, 0, step, seed)
            train_step_noised(model, b, tm, diffusion, yhat=yh[idx], have=hv[idx], stats=acc, count_global=cg, loss=loss, forward_only=True, pool=pool,
                              seed=seed, call_id=EVAL_CALL, offsets=(n0, step * int(batch_size)))
            n0 += sum(_counts(b))
    return acc


def _metrics(model, a):
    """stats (host list, stats_len(P)) -> per-property dict(mse, mae, mse_raw, mae_raw, count)."""
    out = {}
    for p, name in enumerate(model.names):
        s2, sa, n = a[1 + 3 * p], a[2 + 3 * p], a[3 + 3 * p]
        sd = float(model.normalizer.std[p])
        mse, mae = (s2 / n, sa / n) if n > 0 else (float("nan"), float("nan"))
        out[name] = dict(mse=mse, mae=mae, mse_raw=mse * sd * sd, mae_raw=mae * sd, count=int(round(n)))
    return out


def evaluate(model, data_list, batch_size, pool=None, t=None, diffusion=None, seed=0):
    """Per property: mean squared and mean absolute error over the set's present targets, in normalised units (mse, mae) and in the
    property's own (mse_raw, mae_raw), and the count.  Forward-only; mini-batches are weighted by their counts, so the result does not
    depend on batch_size beyond fp32 summation order.  One host read.
    t (with `diffusion`, the module a noise-aware predictor was trained under): the error at that fixed time 0..T, on inputs noised under
    `seed`; a predictor that is not noised, or one of another schedule, is refused by name."""
    if int(batch_size) < 1:
        raise ValueError(f"evaluate: batch_size = {batch_size}: must be >= 1")
    if len(data_list) == 0:
        raise ValueError("evaluate: an empty set")
    if t is not None:
        if diffusion is None:
            raise ValueError("evaluate: t = needs diffusion = the module whose schedule noises the inputs")
        T = require_noised(model, "evaluate(t=)", diffusion)["T"]
        if not 0 <= int(t) <= T:
            raise ValueError(f"evaluate: t = {t} lies outside 0..{T}")
    elif diffusion is not None:
        raise ValueError("evaluate: diffusion = without t = (the time the error is taken at)")
    was_training = model.training
    model.eval()
    try:
        acc = _eval_enqueue(model, data_list, batch_size, torch.zeros(stats_len(model.P), device=model.device), pool=pool, diffusion=diffusion, t=t,
                            seed=seed)
    finally:
        model.train(was_training)
    return _metrics(model, acc.tolist())


def _refuse_world(where):
    from .dist import rank_world
    world = int(rank_world()[1])
    if world > 1:
        raise ValueError(f"{where}: world size {world}: the predictor trains on one GPU only (data-parallel fit_predictor is out of scope)")


def fit_predictor(model, data_list, cfg, val_list=None, seed=0, log=logging.info, on_epoch_end=None, diffusion=None):
    """Train `model` on `data_list` (CrystalData records carrying `properties`).  cfg (key or attribute access): lr, epochs, batch_size;
    accum_steps (default 1); shuffle (default true); loss = "mse" (default) or "l1"; max_grad_norm / skip_nonfinite_steps; lr_plateau;
    handle_pool; ema -- all as pretrain.fit reads them, and with its machinery: epochs of pretrain.batch_plan mini-batches (the only random
    thing, a function of (seed, epoch)), one FusedAdam on the flat vector, one host read per epoch.  The normaliser is fitted on the
    training set first.  With ema the optimizer is left in model.fit_optimizer (ema_weights(model) to predict or save the average).
    diffusion (a DiffCSPModule): the NOISE-AWARE predictor -- every crystal of every mini-batch is forward-noised at one time
    drawn uniformly in 0..T, a function of (seed, epoch, step) (draw_noised_times), under the module's schedule tables; the noise is Philox
    draws 7-9 under `seed` at a call id that counts the micro-steps from 1; the validation set is noised the same way every epoch.  T and
    the schedule's parameters are recorded in model.hparams["noised"] (saved and loaded with the model).
    One GPU only: a world size above 1 is a ValueError.  Returns the per-epoch dicts: train_loss, train_mse_<name>, with a validation set
    val_loss and val_mse_<name> / val_mae_<name> (normalised units), lr, the optimizer's statistics."""
    _refuse_world("fit_predictor")
    from .data import CrystalBatchData
    from .finetune import _epoch_reduce
    from .optim import FusedAdam, cfg_get, clip_options, ema_decay_at, epoch_grad_stats, parse_ema, window_closes
    from .pool import HandlePool, parse_handle_pool
    from .pretrain import batch_plan, plateau_scheduler
    v = {k: cfg_get(cfg, k) for k in ("lr", "epochs", "batch_size")}
    for k, x in v.items():
        if x is None:
            raise KeyError(f"fit_predictor: the config has no {k}")
    lr, epochs, batch_size = float(v["lr"]), int(v["epochs"]), int(v["batch_size"])
    if batch_size < 1:
        raise ValueError(f"fit_predictor: batch_size = {batch_size}: must be >= 1")
    if len(data_list) == 0:
        raise ValueError("fit_predictor: an empty training set")
    if val_list is not None and len(val_list) == 0:
        raise ValueError("fit_predictor: an empty validation set (pass None for no validation)")
    accum = int(cfg_get(cfg, "accum_steps", 1))
    if accum < 1:
        raise ValueError(f"fit_predictor: accum_steps = {accum}: must be >= 1")
    loss = str(cfg_get(cfg, "loss", "mse"))
    if loss not in LOSS_KINDS:
        raise ValueError(f"fit_predictor: loss = {loss!r}: it takes 'mse' or 'l1'")
    shuffle = bool(cfg_get(cfg, "shuffle", True))
    opt = clip_options(cfg)
    pool_kw = parse_handle_pool(cfg_get(cfg, "handle_pool"))
    ema = parse_ema(cfg_get(cfg, "ema"))
    nm = PropertyNormalizer(model.names).fit(data_list)
    if not np.isfinite(nm.raw(data_list)).any():
        raise ValueError(f"fit_predictor: no training crystal carries any of the properties {model.names} (CrystalData.properties)")
    model.set_normalizer(nm)
    T_noise = None
    if diffusion is None:
        model.hparams.pop("noised", None)   # (trained on clean inputs from here on: no longer a noise-aware predictor)
    else:
        model.hparams["noised"] = noised_spec(diffusion)
        T_noise = model.hparams["noised"]["T"]
        calls = 0
    if ema is not None:
        opt = dict(opt, ema_decay=ema["decay"], ema_warmup=ema["warmup"])
    flat = model.flat
    optimizer = FusedAdam([flat], lr=lr, **opt)
    plateau = plateau_scheduler(optimizer, cfg_get(cfg, "lr_plateau"))
    if flat.grad is None:
        flat.grad = torch.zeros_like(flat)
    if ema is not None:
        model.__dict__["fit_optimizer"] = optimizer
    dev, P, n = model.device, model.P, len(data_list)
    yh, hv = nm(data_list)
    pool = None if pool_kw is None else HandlePool(**pool_kw)
    out = []
    try:
        for epoch in range(epochs):
            model.train()
            optimizer.zero_grad(set_to_none=False)
            acc = torch.zeros(stats_len(P), device=dev)
            plan = batch_plan(n, batch_size, epoch, seed, shuffle)
            for step, idx in enumerate(plan):
                if diffusion is None:
                    train_step(model, CrystalBatchData([data_list[i] for i in idx]), yhat=yh[idx], have=hv[idx], grad=flat.grad, stats=acc,
                               accum_steps=accum, loss=loss, pool=pool)
                else:
                    calls += 1
                    train_step_noised(model, CrystalBatchData([data_list[i] for i in idx]), draw_noised_times(len(idx), T_noise, epoch, step, seed),
                                      diffusion, yhat=yh[idx], have=hv[idx], grad=flat.grad, stats=acc, accum_steps=accum, loss=loss, pool=pool,
                                      seed=seed, call_id=calls)
                if window_closes(step + 1, accum, len(plan)):
                    optimizer.step()
                    optimizer.zero_grad(set_to_none=False)
            if val_list is not None:
                with optimizer.ema_weights(model) if ema is not None and ema["validate"] else contextlib.nullcontext():
                    acc = torch.cat([acc, _eval_enqueue(model, val_list, batch_size, torch.zeros(stats_len(P), device=dev), loss=loss, pool=pool,
                                                          diffusion=diffusion, seed=seed)])
            k_ema = None
            if ema is not None and optimizer.guarded:
                k_ema = acc.numel()
                acc = torch.cat([acc, optimizer.adam_steps()])
            a = _epoch_reduce(acc, "fit_predictor", optimizer)   # the epoch's only host read
            s_ema = None
            if k_ema is not None:
                s_ema = int(round(a.pop(k_ema)))
            elif ema is not None:
                s_ema = int(optimizer.state[flat]["step"])
            d = dict(train_loss=a[0] / len(plan))
            for name, m in _metrics(model, a[:stats_len(P)]).items():
                d[f"train_mse_{name}"] = m["mse"]
            k = stats_len(P)
            if val_list is not None:
                d["val_loss"] = a[k]
                for name, m in _metrics(model, a[k:2 * k]).items():
                    d[f"val_mse_{name}"], d[f"val_mae_{name}"] = m["mse"], m["mae"]
                k *= 2
            d["lr"] = float(optimizer.param_groups[0]["lr"])
            if len(a) > k:
                d.update(epoch_grad_stats(a[k:]))
            if ema is not None:
                d["ema_decay"] = ema_decay_at(ema["decay"], ema["warmup"], s_ema)
            if plateau is not None:
                plateau.step(d["val_loss"] if val_list is not None else d["train_loss"])
            out.append(d)
            log(f"Epoch {epoch}: " + ", ".join(f"{k_}: {v_:.6g}" for k_, v_ in d.items()))
            if on_epoch_end is not None:
                on_epoch_end(epoch, d)
    finally:
        if pool is not None:
            model.__dict__["handle_pool_stats"] = pool.stats()
            pool.close()
    return out


# ---- model directories ------------------------------------------------------------------------------------------
def write_hparams(save_dir, hparams, normalizer):
    os.makedirs(save_dir, exist_ok=True)
    hp = {k: hparams[k] for k in HPARAM_KEYS}
    hp.update(mean=[float(x) for x in normalizer.mean], std=[float(x) for x in normalizer.std])
    if hparams.get("noised") is not None:   # (a noise-aware predictor; a directory without the entry loads with noised = None)
        hp["noised"] = hparams["noised"]
    CFG.save(CFG.create({"predictor": hp}), os.path.join(save_dir, HPARAMS_FILE))


def read_hparams(model_dir, names=None):
    """The `predictor` entry of <model_dir>/hparams.yaml as a dict.  names: the properties the caller expects, in order; a saved model
    whose names differ is refused (ValueError naming both lists) before any weight is read."""
    path = os.path.join(str(model_dir), HPARAMS_FILE)
    if not os.path.exists(path):
        raise FileNotFoundError(f"load_predictor: {path} does not exist")
    cfg = CFG.to_container(CFG.load(path), resolve=True)
    if "predictor" not in cfg:
        raise ValueError(f"load_predictor: {path} has no `predictor` entry (not a directory written by save_predictor)")
    hp = dict(cfg["predictor"])
    hp["names"] = [str(n) for n in hp["names"]]
    if names is not None and _names(names) != hp["names"]:
        raise ValueError(f"load_predictor: the saved model's names {hp['names']} differ from the expected names {_names(names)}")
    return hp


def save_predictor(model, save_dir):
    """<save_dir>/hparams.yaml (the constructor's arguments and the normaliser) + last.ckpt ({"state_dict"}: scalar_out.*, then the trunk)."""
    write_hparams(save_dir, model.hparams, model.normalizer)
    torch.save({"state_dict": {k: v.cpu() for k, v in model.state_dict().items()}}, os.path.join(save_dir, WEIGHTS_FILE))
    return save_dir


def load_predictor(model_dir, device=None, names=None):
    """The inverse of save_predictor.  names: see read_hparams."""
    hp = read_hparams(model_dir, names)
    nm = PropertyNormalizer(hp["names"], hp.get("mean"), hp.get("std"))
    model = PropertyPredictor(normalizer=nm, device=device, **{k: hp[k] for k in HPARAM_KEYS})
    if hp.get("noised") is not None:
        nz = dict(hp["noised"])
        model.hparams["noised"] = dict(T=int(nz["T"]), beta_scheduler=dict(nz.get("beta_scheduler") or {}), sigma_scheduler=dict(nz.get("sigma_scheduler") or {}))
    ck = torch.load(os.path.join(str(model_dir), WEIGHTS_FILE), map_location="cpu", weights_only=False)
    model.load_state_dict(ck["state_dict"])
    return model

"""Fused Adam on the flat parameter vector (mi_adam_step).

Same update as `torch.optim.Adam(params, lr)` with its defaults, which is what
MatInvent.ft_step constructs (pipeline/mat_invent.py:136): beta=(0.9, 0.999), eps=1e-8, no
weight decay, no amsgrad, bias-corrected; state starts at zero.  One kernel over one buffer.

`max_grad_norm` / `skip_nonfinite` (both off by default, and then nothing below this line is used): the step becomes mi_grad_norm +
mi_adam_step_guarded (include/matinvent_hip_optim.h).  The gradient's global norm is reduced on the device in a fixed order
(same bits every call), the gradient is scaled by torch.nn.utils.clip_grad_norm_'s coefficient inside the Adam pass, and a step whose
norm is inf / NaN is left out altogether -- parameters, moments and Adam's bias-correction count keep their bits -- without the host
ever waiting: whether a step was applied is known to the device only, so the applied-step count lives there.  Clipping alone does not
guard: with skip_nonfinite=False a NaN gradient reaches the parameters as it does in torch.

Several ranks: the norm is taken inside step(), after the caller's all-reduce of the gradient, so every rank reduces the same buffer in
the same order and arrives at the same coefficient and the same decision; every rank (one with an empty shard too) must construct its
optimizer with the same options.

`ema_decay` (off by default, and then no call changes): every step is mi_adam_step_ema (include/matinvent_hip_ema.h), behind
mi_grad_norm when guarded -- Adam's update and ema = d_s ema + (1 - d_s) theta_new in ONE pass over the flat vector.  The average follows
the guard: a skipped step leaves it alone and does not advance the warm-up of its decay (ema_decay_at), which counts applied steps.
`ema_weights` swaps the average into the network; state_dict / load_state_dict carry it and the device's state block.
"""
import contextlib
import math
import numbers

import numpy as np

import torch

from . import _lib
from .cspnet import _ptr, _stream

# grad_stats(): one float64 value per name
GRAD_STATS = ("applied_steps", "skipped_steps", "clipped_steps", "nonfinite_steps", "last_norm", "last_coef", "norm_sum", "norm_max")
# the state block's words (include/matinvent_hip_optim.h)
_W_COEF, _W_ADAM_STEPS, _W_COUNTS, _W_LAST_NORM, _W_NORM_MAX, _W_STATS_END, _D_NORM_SUM = 0, 4, 5, 9, 10, 14, 6


def cfg_get(cfg, k, default=None):
    """Entry `k` of a fine-tune config with key or attribute access (a dict, a namespace, a DictConfig); `default` when absent or None."""
    v = cfg.get(k) if isinstance(cfg, dict) else getattr(cfg, k, None)
    if v is None and not isinstance(cfg, dict) and hasattr(cfg, "get"):
        v = cfg.get(k, None)
    return default if v is None else v


def window_closes(done, accum_steps, total):
    """The optimizer steps once `done` of an epoch's `total` micro-steps are enqueued: at the end of every accumulation window of
    `accum_steps`, and behind the last micro-step when that leaves a window partly filled (pipeline/mat_invent.py:165-167, :176-177)."""
    return done % accum_steps == 0 or done == total


def clip_options(cfg):
    """The optimizer options of a fine-tune config (key or attribute access): `max_grad_norm` (a number > 0, +inf included; None / absent:
    no clipping) and `skip_nonfinite_steps` (bool; None / absent: False) -> FusedAdam's keyword arguments.  ValueError, naming the key,
    for anything else: a negative number, zero, NaN, a bool or a string as max_grad_norm; a non-bool as skip_nonfinite_steps."""
    m = cfg_get(cfg, "max_grad_norm")
    if m is not None:
        if isinstance(m, bool) or not isinstance(m, numbers.Real) or math.isnan(m) or not m > 0:
            raise ValueError(f"max_grad_norm = {m!r}: must be a number > 0 (or None: no clipping)")
        m = float(m)
    s = cfg_get(cfg, "skip_nonfinite_steps", False)
    if not isinstance(s, bool):
        raise ValueError(f"skip_nonfinite_steps = {s!r}: must be true or false")
    return dict(max_grad_norm=m, skip_nonfinite=s)


def epoch_grad_stats(v):
    """grad_stats() values (a sequence in GRAD_STATS order, on the host) -> the four entries of an epoch's dict: grad_norm (mean norm
    before clipping over the steps whose norm was finite), grad_norm_max, clipped_steps, skipped_steps."""
    s = dict(zip(GRAD_STATS, v))
    finite = s["applied_steps"] + s["skipped_steps"] - s["nonfinite_steps"]
    return dict(grad_norm=s["norm_sum"] / max(1.0, finite), grad_norm_max=s["norm_max"], clipped_steps=int(round(s["clipped_steps"])),
                skipped_steps=int(round(s["skipped_steps"])))


def parse_ema(value):
    """cfg.ema -> None (no average) or dict(decay, warmup, validate): None / absent (the default), a float decay in [0, 1), or a mapping
    {decay, warmup: true, validate: true}.  warmup: the decay of applied step s is min(decay, (1 + s) / (10 + s)).  validate: pretrain.fit's
    validation pass runs on the averaged weights.  Anything else is a ValueError that names `ema`."""
    if value is None:
        return None
    spec = {"decay": value}
    if not isinstance(value, (bool, str, bytes, numbers.Real)):
        if not (hasattr(value, "keys") and hasattr(value, "__getitem__")):
            raise ValueError(f"ema = {value!r}: it takes null, a decay in [0, 1) or {{decay, warmup, validate}}")
        spec = {k: value[k] for k in value.keys()}
        extra = set(spec) - {"decay", "warmup", "validate"}
        if extra:
            raise ValueError(f"ema: unknown key(s) {sorted(extra)}; it takes decay, warmup, validate")
        if spec.get("decay") is None:
            raise ValueError("ema: a mapping needs `decay`")
    d = spec["decay"]
    if isinstance(d, bool) or not isinstance(d, numbers.Real) or math.isnan(d) or not 0.0 <= d < 1.0:
        raise ValueError(f"ema decay = {d!r}: must be a number in [0, 1)")
    out = {"decay": float(d)}
    for k in ("warmup", "validate"):
        b = spec.get(k)
        b = True if b is None else b
        if not isinstance(b, bool):
            raise ValueError(f"ema.{k} = {b!r}: must be true or false")
        out[k] = b
    return out


def ema_decay_at(ema_decay, ema_warmup, s):
    """d_s, the decay that applied step `s` uses, as csrc/ema_decay.h forms it: the decay rounded to float32 (it crosses the C boundary as
    a float), min with (1 + s) / (10 + s) in float64 under warm-up, rounded to float32 once.  Returned as a Python float."""
    d = float(np.float32(ema_decay))
    return float(np.float32(min(d, (1.0 + int(s)) / (10.0 + int(s))))) if ema_warmup else d


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, skip_nonfinite=False, ema_decay=None, ema_warmup=True):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self._lib = _lib.load()
        opts = clip_options(dict(max_grad_norm=max_grad_norm, skip_nonfinite_steps=skip_nonfinite))
        self.max_grad_norm, self.skip_nonfinite = opts["max_grad_norm"], opts["skip_nonfinite"]
        self.guarded = self.max_grad_norm is not None or self.skip_nonfinite
        e = parse_ema(None if ema_decay is None else dict(decay=ema_decay, warmup=ema_warmup))
        self.ema_decay, self.ema_warmup = (None, True) if e is None else (e["decay"], e["warmup"])
        self.ema, self._ema_swapped = None, False   # the average: a copy of theta taken at the first step(), before the update
        if self.guarded or self.ema_decay is not None:
            ps = [p for g in self.param_groups for p in g["params"]]
            if len(ps) != 1:
                raise ValueError("FusedAdam: max_grad_norm / skip_nonfinite / ema_decay work on ONE flat parameter vector, got "
                                 f"{len(ps)} parameters")
            p = ps[0]
        if self.guarded:
            assert self._lib.mi_optim_state_bytes() == 64
            # the device's state block (zeroed once, then written by the device only) and the reduction's per-block sums
            self._opt_state = torch.zeros(16, dtype=torch.int32, device=p.device)
            self._opt_work = torch.empty(self._lib.mi_optim_workspace_bytes(p.numel()) // 4, dtype=torch.float32, device=p.device)   # (holds doubles)

    def grad_stats(self, reset=False):
        """The running statistics of the guarded step as a float64 device tensor in GRAD_STATS order, enqueued on the current stream with
        no host synchronisation: the caller decides when to read it.  reset=True starts a new period behind it (Adam's own step count
        is not a statistic and stays)."""
        if not self.guarded:
            raise RuntimeError("FusedAdam.grad_stats: neither max_grad_norm nor skip_nonfinite is set")
        st = self._opt_state
        f32, f64 = st.view(torch.float32), st.view(torch.float64)
        out = torch.cat([st[_W_COUNTS:_W_COUNTS + 4].double(), f32[_W_LAST_NORM:_W_LAST_NORM + 1].double(), f32[_W_COEF:_W_COEF + 1].double(),
                         f64[_D_NORM_SUM:_D_NORM_SUM + 1], f32[_W_NORM_MAX:_W_NORM_MAX + 1].double()])
        if reset:
            st[_W_COUNTS:_W_STATS_END].zero_()
        return out

    def options(self):
        """What a checkpoint must find unchanged (load_state_dict; pretrain.fit's resume)."""
        return dict(max_grad_norm=self.max_grad_norm, skip_nonfinite=self.skip_nonfinite, ema_decay=self.ema_decay,
                    ema_warmup=self.ema_warmup if self.ema_decay is not None else None)

    def _flat(self):
        return self.param_groups[0]["params"][0]

    def adam_steps(self):
        """The device's count of applied steps (Adam's bias-correction count under the guard) as a float32 device tensor of one element, with
        no host synchronisation."""
        if not self.guarded:
            raise RuntimeError("FusedAdam.adam_steps: neither max_grad_norm nor skip_nonfinite is set (the host's state['step'] is the count)")
        return self._opt_state[_W_ADAM_STEPS:_W_ADAM_STEPS + 1].to(torch.float32)

    @contextlib.contextmanager
    def ema_weights(self, owner=None):
        """Inside the context the network holds the averaged weights: theta and the average exchange their contents and `owner` (default:
        the network theta belongs to) is told that its packed weights are stale, on entry and on exit.  Every forward, evaluate, sample and
        save_model inside sees the average.  Not re-entrant; step() inside raises.  Before the first step the average IS theta."""
        if self.ema_decay is None:
            raise RuntimeError("FusedAdam.ema_weights: ema_decay is not set")
        if self._ema_swapped:
            raise RuntimeError("FusedAdam.ema_weights: already inside (not re-entrant)")
        p = self._flat()
        owner = getattr(p, "_mi_owner", None) if owner is None else owner

        def swap():
            if self.ema is not None:
                with torch.no_grad():
                    t = p.data.clone()
                    p.data.copy_(self.ema)
                    self.ema.copy_(t)
            if owner is not None:
                owner.mark_dirty()
        swap()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._ema_swapped = False
            swap()

    def state_dict(self):
        """torch's state_dict (step, exp_avg, exp_avg_sq, param_groups) plus "fused": the options, the parameter's length, the average and
        the device's 16-word state block (adam_steps, Adam's bias-correction count under the guard, lives there).  Tensors are copies."""
        if self._ema_swapped:
            raise RuntimeError("FusedAdam.state_dict: inside ema_weights (theta and the average are exchanged)")
        sd = super().state_dict()
        sd["state"] = {k: {n: (v.detach().clone() if torch.is_tensor(v) else v) for n, v in st.items()} for k, st in sd["state"].items()}
        sd["fused"] = dict(options=self.options(), numel=sum(p.numel() for g in self.param_groups for p in g["params"]),
                           ema=None if self.ema is None else self.ema.detach().clone(),
                           opt_state=self._opt_state.detach().clone() if self.guarded else None)
        return sd

    def load_state_dict(self, state_dict):
        """The inverse of state_dict.  ValueError when this optimizer's guard / average options differ from the saved ones, or the
        parameter's length does: continuing would silently be another run."""
        f = state_dict.get("fused")
        if f is None:
            raise ValueError("FusedAdam.load_state_dict: not a FusedAdam state_dict (no 'fused' entry)")
        mine = self.options()
        for k, v in f["options"].items():
            if mine[k] != v:
                raise ValueError(f"FusedAdam.load_state_dict: option {k} = {mine[k]!r} here, {v!r} in the saved state")
        numel = sum(p.numel() for g in self.param_groups for p in g["params"])
        if numel != f["numel"]:
            raise ValueError(f"FusedAdam.load_state_dict: numel = {numel} parameters here, {f['numel']} in the saved state")
        if self._ema_swapped:
            raise RuntimeError("FusedAdam.load_state_dict: inside ema_weights")
        super().load_state_dict({k: v for k, v in state_dict.items() if k != "fused"})
        if self.guarded:
            self._opt_state.copy_(f["opt_state"])
        if self.ema_decay is not None:
            p = self._flat()
            self.ema = None if f["ema"] is None else f["ema"].detach().to(p.device, torch.float32).clone()

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0):
        if self._ema_swapped:
            raise RuntimeError("FusedAdam.step: inside ema_weights (theta holds the average)")
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                assert p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.grad.is_contiguous()
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
                st["step"] += 1   # attempted steps; with skip_nonfinite the device counts the applied ones
                if self.guarded:
                    _lib.check(self._lib.mi_grad_norm(_ptr(p.grad), p.numel(), grad_scale, self.max_grad_norm or 0.0, int(self.skip_nonfinite),
                                                      group["lr"], b1, b2, _ptr(self._opt_state), _ptr(self._opt_work), _stream()), "mi_grad_norm")
                if self.ema_decay is not None:
                    if self.ema is None:
                        self.ema = p.data.clone()
                    _lib.check(self._lib.mi_adam_step_ema(_ptr(p.data), _ptr(p.grad), _ptr(st["exp_avg"]), _ptr(st["exp_avg_sq"]), _ptr(self.ema),
                                                          p.numel(), st["step"], group["lr"], b1, b2, group["eps"], grad_scale, self.ema_decay,
                                                          int(self.ema_warmup), _ptr(self._opt_state) if self.guarded else None, _stream()),
                               "mi_adam_step_ema")
                elif self.guarded:
                    _lib.check(self._lib.mi_adam_step_guarded(_ptr(p.data), _ptr(p.grad), _ptr(st["exp_avg"]), _ptr(st["exp_avg_sq"]), p.numel(),
                                                              b1, b2, group["eps"], grad_scale, _ptr(self._opt_state), _stream()),
                               "mi_adam_step_guarded")
                else:
                    _lib.check(self._lib.mi_adam_step(_ptr(p.data), _ptr(p.grad), _ptr(st["exp_avg"]), _ptr(st["exp_avg_sq"]), p.numel(),
                                                      st["step"], group["lr"], b1, b2, group["eps"], grad_scale, _stream()), "mi_adam_step")
                owner = getattr(p, "_mi_owner", None)
                if owner is not None:
                    owner.mark_dirty()  # packed weight copies are stale now

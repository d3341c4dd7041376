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
"""
import math
import numbers

import torch

from . import _lib
from .cspnet import _ptr, _stream

# grad_stats(): one float64 value per name
GRAD_STATS = ("applied_steps", "skipped_steps", "clipped_steps", "nonfinite_steps", "last_norm", "last_coef", "norm_sum", "norm_max")
# the state block's words (include/matinvent_hip_optim.h)
_W_COEF, _W_COUNTS, _W_LAST_NORM, _W_NORM_MAX, _W_STATS_END, _D_NORM_SUM = 0, 5, 9, 10, 14, 6


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


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, skip_nonfinite=False):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self._lib = _lib.load()
        opts = clip_options(dict(max_grad_norm=max_grad_norm, skip_nonfinite_steps=skip_nonfinite))
        self.max_grad_norm, self.skip_nonfinite = opts["max_grad_norm"], opts["skip_nonfinite"]
        self.guarded = self.max_grad_norm is not None or self.skip_nonfinite
        if self.guarded:
            ps = [p for g in self.param_groups for p in g["params"]]
            if len(ps) != 1:
                raise ValueError(f"FusedAdam: max_grad_norm / skip_nonfinite take the norm of ONE flat parameter vector, got {len(ps)} parameters")
            p = ps[0]
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

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0):
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
                    _lib.check(self._lib.mi_adam_step_guarded(_ptr(p.data), _ptr(p.grad), _ptr(st["exp_avg"]), _ptr(st["exp_avg_sq"]), p.numel(),
                                                              b1, b2, group["eps"], grad_scale, _ptr(self._opt_state), _stream()),
                               "mi_adam_step_guarded")
                else:
                    _lib.check(self._lib.mi_adam_step(_ptr(p.data), _ptr(p.grad), _ptr(st["exp_avg"]), _ptr(st["exp_avg_sq"]), p.numel(),
                                                      st["step"], group["lr"], b1, b2, group["eps"], grad_scale, _stream()), "mi_adam_step")
                owner = getattr(p, "_mi_owner", None)
                if owner is not None:
                    owner.mark_dirty()  # packed weight copies are stale now

"""CPU-only checks of the optimizer extension (include/matinvent_hip_optim.h, matinvent_amd.optim): the config validation helper, the
host-only size functions, and the refusals that happen before anything is enqueued.  No device is touched."""
import ctypes as C
import math

import numpy as np
import pytest

from matinvent_amd import _lib
from matinvent_amd.build import build
from matinvent_amd.optim import GRAD_STATS, clip_options, epoch_grad_stats


class _Attr:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.mark.parametrize("cfg,want", [
    ({}, dict(max_grad_norm=None, skip_nonfinite=False)),
    (dict(lr=1e-4), dict(max_grad_norm=None, skip_nonfinite=False)),
    (dict(max_grad_norm=None, skip_nonfinite_steps=None), dict(max_grad_norm=None, skip_nonfinite=False)),
    (dict(max_grad_norm=1.0), dict(max_grad_norm=1.0, skip_nonfinite=False)),
    (dict(max_grad_norm=2), dict(max_grad_norm=2.0, skip_nonfinite=False)),
    (dict(max_grad_norm=np.float32(0.5)), dict(max_grad_norm=0.5, skip_nonfinite=False)),
    (dict(max_grad_norm=1e-30, skip_nonfinite_steps=True), dict(max_grad_norm=1e-30, skip_nonfinite=True)),
    (dict(max_grad_norm=math.inf), dict(max_grad_norm=math.inf, skip_nonfinite=False)),
    (dict(skip_nonfinite_steps=True), dict(max_grad_norm=None, skip_nonfinite=True)),
    (dict(skip_nonfinite_steps=False), dict(max_grad_norm=None, skip_nonfinite=False)),
])
def test_clip_options_accepts(cfg, want):
    from matinvent_amd import config
    for c in (cfg, _Attr(**cfg), config.create(cfg)):
        got = clip_options(c)
        assert got == want and (got["max_grad_norm"] is None or type(got["max_grad_norm"]) is float)


@pytest.mark.parametrize("cfg,key", [
    (dict(max_grad_norm=-1.0), "max_grad_norm"),
    (dict(max_grad_norm=0), "max_grad_norm"),
    (dict(max_grad_norm=0.0), "max_grad_norm"),
    (dict(max_grad_norm=float("nan")), "max_grad_norm"),
    (dict(max_grad_norm=-math.inf), "max_grad_norm"),
    (dict(max_grad_norm="1.0"), "max_grad_norm"),
    (dict(max_grad_norm=True), "max_grad_norm"),
    (dict(max_grad_norm=[1.0]), "max_grad_norm"),
    (dict(skip_nonfinite_steps=1), "skip_nonfinite_steps"),
    (dict(skip_nonfinite_steps="yes"), "skip_nonfinite_steps"),
    (dict(max_grad_norm=1.0, skip_nonfinite_steps=0.0), "skip_nonfinite_steps"),
])
def test_clip_options_refuses_and_names_the_key(cfg, key):
    for c in (cfg, _Attr(**cfg)):
        with pytest.raises(ValueError, match=key):
            clip_options(c)


def test_epoch_grad_stats_mean_is_over_the_finite_norms():
    v = dict(applied_steps=4, skipped_steps=1, clipped_steps=3, nonfinite_steps=1, last_norm=2.0, last_coef=0.5, norm_sum=10.0, norm_max=4.0)
    d = epoch_grad_stats([v[k] for k in GRAD_STATS])
    assert d == dict(grad_norm=2.5, grad_norm_max=4.0, clipped_steps=3, skipped_steps=1)
    assert epoch_grad_stats([0.0] * len(GRAD_STATS))["grad_norm"] == 0.0      # an epoch without a step


def test_size_functions_need_no_device():
    build(verbose=False)
    lib = _lib.load()
    assert lib.mi_optim_state_bytes() == 64
    cap = lib.mi_optim_sweep_elems(1 << 40)                 # the capped grid's elements per sweep
    assert cap > 0 and cap % 4 == 0
    per_block = lib.mi_optim_sweep_elems(1)                 # one block
    assert 0 < per_block <= cap and cap % per_block == 0
    assert lib.mi_optim_sweep_elems(0) == per_block and lib.mi_optim_workspace_bytes(0) == 8
    for n in (1, per_block, per_block + 1, 100003, cap - 1, cap, cap + 1, 12346468, 1 << 33):
        blocks = lib.mi_optim_sweep_elems(n) // per_block
        assert blocks == min(-(-n // per_block), cap // per_block)      # a function of n alone, capped
        assert lib.mi_optim_workspace_bytes(n) == 8 * blocks
    assert lib.mi_optim_workspace_bytes(-1) == _lib.MI_EINVAL and lib.mi_optim_sweep_elems(-5) == _lib.MI_EINVAL


def test_refusals_before_anything_is_enqueued():
    """NULL pointers, a negative n and a NaN max_norm return MI_EINVAL; the pointers are host dummies that a refused call never reads."""
    build(verbose=False)
    lib = _lib.load()
    buf = (C.c_double * 16)()
    p = C.c_void_p(C.addressof(buf))
    good = dict(grad=p, n=4, scale=1.0, max_norm=1.0, skip=1, lr=1e-3, b1=0.9, b2=0.999, state=p, work=p)

    def norm(**kw):
        a = dict(good, **kw)
        return lib.mi_grad_norm(a["grad"], a["n"], a["scale"], a["max_norm"], a["skip"], a["lr"], a["b1"], a["b2"], a["state"], a["work"], None)

    for k in ("grad", "state", "work"):
        assert norm(**{k: None}) == _lib.MI_EINVAL, k
        assert b"null" in lib.mi_last_error()
    assert norm(n=-1) == _lib.MI_EINVAL and b"n = -1" in lib.mi_last_error()
    assert norm(max_norm=float("nan")) == _lib.MI_EINVAL and b"NaN" in lib.mi_last_error()

    def adam(theta=p, grad=p, m=p, v=p, n=4, state=p):
        return lib.mi_adam_step_guarded(theta, grad, m, v, n, 0.9, 0.999, 1e-8, 1.0, state, None)

    for k in ("theta", "grad", "m", "v", "state"):
        assert adam(**{k: None}) == _lib.MI_EINVAL, k
    assert adam(n=-3) == _lib.MI_EINVAL and b"n = -3" in lib.mi_last_error()
    assert adam(n=0) == 0                                    # nothing to do, nothing enqueued

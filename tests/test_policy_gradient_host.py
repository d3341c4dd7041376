"""CPU-only checks of the PPO-clipped policy gradient's host side (matinvent_amd.policy): advantage normalisation, the timestep draws,
the surrogate's gradient rule (the arithmetic of mi_traj_pg_step's surrogate kernel, written out in numpy) against torch autograd, and the
drop-in config of the pipeline."""
import os

import numpy as np
import pytest
import torch

from matinvent_amd import config as C
from matinvent_amd import policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "dropin", "configs")


def test_advantages_normalise_clip_and_constant_rewards():
    r = np.array([0.1, 0.4, 0.4, 0.9, 0.2])
    a = policy.advantages(r)
    ref = (r - r.mean()) / (r.std() + 1e-8)                   # population std
    np.testing.assert_allclose(a, ref, rtol=1e-6)
    assert a.dtype == np.float32
    assert abs(float(a.astype(np.float64).mean())) < 1e-6
    # one outlier among many: its normalised advantage exceeds the clip
    r = np.zeros(100)
    r[0] = 1.0
    a = policy.advantages(r, adv_clip=5.0)
    assert a[0] == np.float32(5.0) and np.all(a[1:] < 0)
    a = policy.advantages(r, adv_clip=2.0)
    assert a[0] == np.float32(2.0)
    # std = 0: every advantage is zero, not NaN
    a = policy.advantages(np.full(7, 0.3))
    assert np.all(a == 0) and np.isfinite(a).all()


def test_timestep_draws_distinct_in_range_reproducible_and_capped():
    T, B = 50, 9
    d = policy.draw_timesteps(T, B, 12, epochs=3, seed=4)
    assert len(d) == 3
    for e in d:
        assert e.shape == (12, B) and e.dtype == np.int32 and e.flags.c_contiguous
        assert e.min() >= 2 and e.max() <= T
        for b in range(B):
            assert len(set(e[:, b].tolist())) == 12                   # without replacement, per crystal
    assert not np.array_equal(d[0], d[1])                            # a new draw per epoch
    d2 = policy.draw_timesteps(T, B, 12, epochs=3, seed=4)
    assert all(np.array_equal(x, y) for x, y in zip(d, d2))
    assert not np.array_equal(policy.draw_timesteps(T, B, 12, epochs=1, seed=5)[0], d[0])
    # capped at T - 1: every time of 2..T exactly once per crystal
    full = policy.draw_timesteps(T, B, 10 * T, epochs=1, seed=0)[0]
    assert full.shape == (T - 1, B)
    for b in range(B):
        assert sorted(full[:, b].tolist()) == list(range(2, T + 1))


def _kernel_rule(lp_new, lp_old, A, eps, scale, w):
    """The surrogate kernel's arithmetic (csrc/traj_logprob.hip, traj_pg_surrogate_kernel) in float32 numpy."""
    f = np.float32
    d = (lp_new - lp_old).astype(f)
    rho = np.exp(d).astype(f)
    lo, hi = f(1.0 - eps), f(1.0 + eps)
    rc = np.where(rho < lo, lo, np.where(rho > hi, hi, rho))
    u, c = -A * rho, -A * rc
    L = np.maximum(u, c)
    unclipped = ~((rho < lo) | (rho > hi)) | (u > c)
    g = np.where(unclipped, (f(scale) * -A) * rho, f(0))
    return L, rho, np.stack([f(wk) * g for wk in w]), np.abs(rho - 1) > eps


@pytest.mark.parametrize("eps", [1e-4, 0.2])
def test_surrogate_gradient_rule_matches_autograd(eps):
    g = torch.Generator().manual_seed(3)
    B, M = 400, 1200
    w = (0.5, 1.0, 2.0)
    lp = torch.randn(3, B, generator=g, dtype=torch.float32)
    # log-ratios spread over both sides of the clip band, every ratio at least 1e-2 eps away from its edges
    logr = (torch.rand(B, generator=g) * 6 - 3) * eps
    edge = torch.minimum((logr.exp() - (1 - eps)).abs(), (logr.exp() - (1 + eps)).abs())
    logr = torch.where(edge < 1e-2 * eps, logr + 0.05 * eps, logr)
    lp_new_ref = (w[0] * lp[0] + w[1] * lp[1]) + w[2] * lp[2]
    lp_old = lp_new_ref - logr
    A = torch.randn(B, generator=g)
    A[::7] = 0.0
    x = lp.clone().requires_grad_(True)
    lp_new = w[0] * x[0] + w[1] * x[1] + w[2] * x[2]
    rho = torch.exp(lp_new - lp_old)
    L = torch.maximum(-A * rho, -A * torch.clamp(rho, 1 - eps, 1 + eps))
    (L.sum() / M).backward()
    Lk, rk, gk, clipped = _kernel_rule(lp_new.detach().numpy(), lp_old.numpy(), A.numpy(), eps, 1.0 / M, w)
    np.testing.assert_allclose(Lk, L.detach().numpy(), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(gk, x.grad.numpy(), rtol=1e-5, atol=1e-12)
    assert clipped.any() and (~clipped).any()
    # the rule's zero: a clipped ratio whose clipped term is the larger one gets no gradient
    sel = clipped & ~(((rk > 1) & (A.numpy() < 0)) | ((rk < 1) & (A.numpy() > 0)))
    assert sel.any() and np.all(gk[:, sel] == 0) and np.all(x.grad.numpy()[:, sel] == 0)


def test_dropin_pg_config_composes():
    cfg = C.resolved(C.compose(EXAMPLE, "base", ["pipeline=mat_invent_pg", "eval_size=6", "device=cuda:0"]))
    p = cfg.pipeline
    assert p._target_ == "pipeline.mat_invent_pg.MatInventPG"
    assert p.replay is False and "topk_ratio" not in p
    ft = p.finetune_cfg
    assert ft.clip_range == pytest.approx(0.2) == policy.DEFAULTS["clip_range"] and ft.adv_clip == 5.0 and list(ft.logprob_weights) == [1.0, 1.0, 1.0]
    assert ft.accum_steps >= 1 and ft.epochs >= 1 and ft.timesteps >= 1
    assert p.sample_cfg == {"num_batches": 1, "max_num": 6}
    merged = C.merge(cfg.model.finetune_cfg, ft)      # what ReinL hands pg_step: lr from the model config
    assert merged.lr == 0.0001
    import sys
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        from pipeline.mat_invent_pg import MatInventPG
        from matinvent_amd.pipeline import MatInvent
        assert issubclass(MatInventPG, MatInvent)
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))


class _Suite:
    sample_cfg = C.create({"batch_size": 4, "num_batches": 1})
    finetune_cfg = C.create({"lr": 1e-4})


@pytest.mark.parametrize("case", ["replay", "mattergen", "world", "num_batches"])
def test_pipeline_refusals(case, monkeypatch, tmp_path):
    """MatInventPG refuses what it does not support before it loads a model."""
    from matinvent_amd import pipeline
    from matinvent_amd.suite import MatterGenSuite
    kw = dict(rl_epoch=1, model_suite=_Suite(), reward=None, sample_cfg={}, finetune_cfg={}, save_dir=str(tmp_path), device="cpu")
    match = {"replay": "replay", "mattergen": "MatterGen", "world": "world_size", "num_batches": "num_batches"}[case]
    if case == "replay":
        kw["replay"] = True
    elif case == "mattergen":
        kw["model_suite"] = MatterGenSuite.__new__(MatterGenSuite)
    elif case == "world":
        monkeypatch.setattr(pipeline, "rank_world", lambda: (0, 2))
    else:
        kw["sample_cfg"] = {"num_batches": 3}
    with pytest.raises(ValueError, match=match):
        pipeline.MatInventPG(**kw)


def test_pg_header_is_exported_and_bound_in_its_own_table():
    import ctypes
    from matinvent_amd import _lib
    from matinvent_amd.build import build
    from tests.header_util import declared_symbols
    names = declared_symbols("matinvent_hip_pg.h")
    assert names == ["mi_traj_pg_step"]
    lib = ctypes.CDLL(build(verbose=False))
    assert hasattr(lib, "mi_traj_pg_step")
    assert sorted(_lib.PG_SIGNATURES) == names and not set(names) & (set(_lib.SIGNATURES) | set(_lib.TRAJ_SIGNATURES))
    bound = _lib.load()
    assert bound.mi_traj_pg_step.argtypes == _lib.PG_SIGNATURES["mi_traj_pg_step"][1]
    # refused on the host, before any device work: null handles
    z = [None] * 21
    assert bound.mi_traj_pg_step(*z[:4], 20, *z[5:14], 0.1, None, 1.0, None, None, None, None) == -1
    assert b"null handle" in bound.mi_last_error()

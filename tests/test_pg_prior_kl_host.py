"""CPU-only checks of the KL anchor of the policy gradient (mi_traj_pg_kl_step, policy.pg_step's kl_coef): the header and its binding,
host refusals, the drop-in config, and the closed-form transition KL (tests/kl_util.py, the restatement the GPU tests use) against torch's
Normal KL, the wrapped-normal KL and autograd in float64."""
import ctypes
import os

import numpy as np
import pytest
import torch

from matinvent_amd import config as C
from matinvent_amd import policy
from tests import kl_util
from tests.header_util import declared_symbols as _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "dropin", "configs")


def test_kl_header_is_exported_and_bound_in_its_own_table():
    from matinvent_amd import _lib
    from matinvent_amd.build import build
    names = _declared("matinvent_hip_pg_kl.h")
    assert names == ["mi_traj_pg_kl_step"]
    lib = ctypes.CDLL(build(verbose=False))
    assert hasattr(lib, "mi_traj_pg_kl_step")
    assert sorted(_lib.PG_KL_SIGNATURES) == names
    assert not set(names) & (set(_lib.SIGNATURES) | set(_lib.TRAJ_SIGNATURES) | set(_lib.PG_SIGNATURES))
    assert _declared("matinvent_hip_pg.h") == ["mi_traj_pg_step"]
    bound = _lib.load()
    assert bound.mi_traj_pg_kl_step.argtypes == _lib.PG_KL_SIGNATURES["mi_traj_pg_kl_step"][1]
    # refused on the host, before any device work: null handles
    z = [None] * 26
    assert bound.mi_traj_pg_kl_step(*z[:6], 20, *z[7:16], 0.1, None, 1.0, 0.1, *z[20:]) == -1
    assert b"null handle" in bound.mi_last_error()


@pytest.mark.parametrize("kl_coef,prior,match", [(0.1, None, "prior"), (-0.5, object(), "kl_coef"), (float("nan"), object(), "kl_coef")])
def test_pg_step_refuses_bad_kl_arguments(kl_coef, prior, match):
    """kl_coef > 0 needs a prior; a negative (or NaN) kl_coef is refused -- both before the agent or the rollout is touched."""
    cfg = dict(lr=1e-4, epochs=1, timesteps=2, accum_steps=1, kl_coef=kl_coef)
    with pytest.raises(ValueError, match=match):
        policy.pg_step(None, None, [0.1, 0.2], cfg, prior=prior)


def test_dropin_pg_config_composes_with_kl_coef():
    cfg = C.resolved(C.compose(EXAMPLE, "base", ["pipeline=mat_invent_pg", "eval_size=6", "device=cuda:0"]))
    ft = cfg.pipeline.finetune_cfg
    assert ft.kl_coef == 0.0 == policy.DEFAULTS["kl_coef"]
    cfg = C.resolved(C.compose(EXAMPLE, "base", ["pipeline=mat_invent_pg", "eval_size=6", "device=cuda:0",
                                                 "pipeline.finetune_cfg.kl_coef=0.01"]))
    assert cfg.pipeline.finetune_cfg.kl_coef == pytest.approx(0.01)


def _random_case(seed, std_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    na = torch.tensor([1, 4, 7, 3])
    B, N = len(na), int(na.sum())
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(B, generator=g, dtype=torch.float64)
    s = dict(c0=u(1.0, 1.2), c1=u(0.01, 0.3), sigma=u(0.02, 0.5), sqrt_sn=u(0.5, 2.0), step_corr=u(1e-4, 5e-2),
             std_corr=u(0.01, 0.3) * std_scale, step_pred=u(1e-4, 9e-2), std_pred=u(0.01, 0.3) * std_scale)
    pred = dict(pl_a=r(B, 3, 3), pl_p=r(B, 3, 3), pt_a=r(N, 100), pt_p=r(N, 100), pxc_a=r(N, 3) * 20, pxc_p=r(N, 3) * 20,
                pxp_a=r(N, 3) * 20, pxp_p=r(N, 3) * 20)
    return s, na, pred


def test_closed_form_kl_is_the_normal_kl_at_the_nearest_image():
    """KL_l, KL_t: torch's KL of the two Normal transitions (means c0 (v - c1 pred)), averaged like the log-probabilities; KL_x: the Normal KL
    of the two coordinate means at their nearest image on the torus (means (x - step sqrt(sn) pred) % 1)."""
    from torch.distributions import Normal, kl_divergence
    s, na, p = _random_case(0)
    B = len(na)
    batch = torch.repeat_interleave(torch.arange(B), na)
    kl_l, kl_t, kl_x = kl_util.kl_terms(s, na, **p)
    g = torch.Generator().manual_seed(1)
    lat, at = torch.randn(B, 3, 3, generator=g, dtype=torch.float64), torch.randn(int(na.sum()), 100, generator=g, dtype=torch.float64)
    x = torch.rand(int(na.sum()), 3, generator=g, dtype=torch.float64)
    c0, c1, sig = s["c0"], s["c1"], s["sigma"]
    m = lambda pl: c0[:, None, None] * (lat - c1[:, None, None] * pl)
    ref_l = kl_divergence(Normal(m(p["pl_a"]), sig[:, None, None]), Normal(m(p["pl_p"]), sig[:, None, None])).mean(dim=(-1, -2))
    mt = lambda pt: c0[batch][:, None] * (at - c1[batch][:, None] * pt)
    ref_t = torch.zeros(B, dtype=torch.float64).index_add(
        0, batch, kl_divergence(Normal(mt(p["pt_a"]), sig[batch][:, None]), Normal(mt(p["pt_p"]), sig[batch][:, None])).mean(dim=-1)) / na
    ref_x = torch.zeros(B, dtype=torch.float64)
    for step, std, a, q in (("step_corr", "std_corr", "pxc_a", "pxc_p"), ("step_pred", "std_pred", "pxp_a", "pxp_p")):
        k = (s[step] * s["sqrt_sn"])[batch][:, None]
        mu_a, mu_p = (x - k * p[a]) % 1.0, (x - k * p[q]) % 1.0
        near = mu_p + kl_util.min_image(mu_a - mu_p)             # the prior's mean moved to the image nearest the agent's
        sd = s[std][batch][:, None]
        ref_x += torch.zeros(B, dtype=torch.float64).index_add(0, batch, kl_divergence(Normal(near, sd), Normal(mu_p, sd)).mean(dim=-1)) / na
    torch.testing.assert_close(kl_l, ref_l, rtol=1e-12, atol=0)
    torch.testing.assert_close(kl_t, ref_t, rtol=1e-12, atol=0)
    torch.testing.assert_close(kl_x, ref_x, rtol=1e-9, atol=1e-15)
    # the case the minimum image exists for: some coordinate differences exceed half a cell
    k = (s["step_corr"] * s["sqrt_sn"])[batch][:, None]
    assert bool(((k * (p["pxc_a"] - p["pxc_p"])).abs() > 0.5).any())


def test_closed_form_derivatives_match_autograd():
    s, na, p = _random_case(2)
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items() if k.endswith("_a")}
    args = dict(p, **leaves)
    w = (0.5, 1.0, 2.0)
    kl_l, kl_t, kl_x = kl_util.kl_terms(s, na, **args)
    ((w[0] * kl_l + w[1] * kl_t + w[2] * kl_x).sum()).backward()
    g_l, g_t, g_xc, g_xp = kl_util.kl_derivatives(s, na, **p)
    for name, ref, wk in (("pl_a", g_l, w[0]), ("pt_a", g_t, w[1]), ("pxc_a", g_xc, w[2]), ("pxp_a", g_xp, w[2])):
        torch.testing.assert_close(leaves[name].grad, wk * ref, rtol=1e-12, atol=1e-300)


def _wrapped_kl(mu_a, mu_p, std, n=20001, images=12):
    """KL of two wrapped normals of the same std on the unit circle by quadrature (float64)."""
    x = np.linspace(0.0, 1.0, n, endpoint=False)
    k = np.arange(-images, images + 1)[:, None]
    pdf = lambda mu: np.exp(-((x[None, :] - mu + k) ** 2) / (2 * std ** 2)).sum(0) / (np.sqrt(2 * np.pi) * std)
    pa, pp = pdf(mu_a), pdf(mu_p)
    return float(np.mean(pa * np.log(pa / pp)))


@pytest.mark.parametrize("std", [0.02, 0.1, 0.3, 0.45])
def test_nearest_image_kl_bounds_the_wrapped_normal_kl(std):
    """The coordinate term is the KL of the unwrapped Gaussians at the nearest image: an upper bound of the wrapped-normal KL (wrapping both
    with one map cannot increase a KL), tight for std << 1/2 (DESIGN 23 records the ratio at the schedule's largest std)."""
    for d in (1e-3, 0.05, 0.2, 0.45):
        bound = d * d / (2 * std * std)
        exact = _wrapped_kl(0.3 + d, 0.3, std)
        assert exact <= bound * (1 + 1e-9), (std, d, exact, bound)
        if std <= 0.1 and d <= 0.05:
            assert exact >= bound * (1 - (1e-6 if std <= 0.02 else 1e-4)), (std, d, exact, bound)

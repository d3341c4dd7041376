"""CPU checks of the conditioned-chain likelihood that need no GPU: tests/lik_ref64.py -- the float64 yardstick of
tests/test_gpu_cond_likelihood.py -- against an element-by-element evaluation, against the unmasked reference with all-false masks and
against hand values with all-true masks; its fp32 restatement and its KL; Condition.select against slicing; Rollout.select carrying the
condition; the header's symbols; the refusals that remain and the new ValueErrors."""
import ctypes

import numpy as np
import pytest
import torch

from matinvent_amd import _lib
from matinvent_amd.conditioning import Condition, check_likelihood
from oracle import diffcsp_oracle as O
from tests import kl_util, lik_ref64 as LR, traj_ref64 as R
from tests.header_util import declared_symbols

T = 20
SIGMA_BEGIN = 0.005
STEP_LR = 5e-6
NA = [1, 4, 5, 2]
TIMES = torch.tensor([2, T, 11, 2])


def _schedules():
    sn = torch.cat([torch.ones(1), torch.linspace(0.6, 1.4, T)])
    return O.beta_tables(T), O.sigma_tables(T, SIGMA_BEGIN, 0.5, sigmas_norm=sn)


def _case(seed=5):
    """A written state (traj_ref64.build_state) and random non-zero predictions: every term depends on its prediction."""
    s = R.step_scalars(*_schedules(), SIGMA_BEGIN, TIMES, STEP_LR)
    g = torch.Generator().manual_seed(seed)
    state = R.to64(R.build_state(NA, TIMES, s, dict(pred_t=torch.randn(100, generator=g)), seed=seed))
    B, N = len(NA), sum(NA)
    r = lambda *shape: 0.3 * torch.randn(*shape, generator=g, dtype=torch.float64)
    return s, state, (r(N, 3), r(B, 3, 3), r(N, 3), r(N, 100))


def _close(a, b, rtol, what):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    scale = max(1e-300, float(b.abs().max()))
    err = float((a - b).abs().max())
    assert err <= rtol * scale, f"{what}: {err:.3e} > {rtol:.0e} * {scale:.3g}"


@pytest.mark.parametrize("mode", ["mixed", "all", "none"])
def test_masked_logprobs_match_an_element_by_element_evaluation(mode):
    s, state, preds = _case()
    masks = LR.make_masks(NA, mode, seed=1)
    lp, _ = LR.logprobs(s, state, preds, masks)
    ref = LR.elementwise(s, state, preds, masks)
    for k in range(3):
        _close(lp[k], ref[k], 1e-12, f"{mode} log-prob {k}")
    if mode == "mixed":
        kt, kx, kl = masks
        assert kt.any() and (~kt).any() and kx.any() and (~kx).any() and kl.any() and (~kl).any() and not torch.equal(kt, kx)


def test_all_false_masks_are_the_unmasked_reference_exactly():
    s, state, preds = _case()
    masks = LR.make_masks(NA, "none")
    lp, d = LR.logprobs(s, state, preds, masks)
    lp0, d0 = R.logprobs(s, state, preds)
    assert all(torch.equal(a, b) for a, b in zip(lp, lp0)) and all(torch.equal(a, b) for a, b in zip(d, d0))
    _, _, prior = _case(seed=6)
    v, dv = LR.kl(s, NA, preds, prior, masks)
    v0, dv0 = R.kl(s, NA, preds, prior)
    assert all(torch.equal(a, b) for a, b in zip(v, v0)) and all(torch.equal(a, b) for a, b in zip(dv, dv0))


def test_all_true_masks_leave_the_corrector_term_alone():
    """Hand values: lp_l = lp_t = 0, lp_x = the corrector's mean; every predictor derivative 0, dx_corr the unmasked one; the KL's
    lattice and type terms 0, its coordinate term the corrector's."""
    s, state, preds = _case()
    masks = LR.make_masks(NA, "all")
    lp, (dl, dt, dxc, dxp) = LR.logprobs(s, state, preds, masks)
    assert torch.count_nonzero(lp[0]) == 0 and torch.count_nonzero(lp[1]) == 0
    na, batch = R._batch(NA)
    pa = lambda k: s[k][batch][:, None]
    lc, _ = R.wrapped_normal(state["frac_coords_mid"], (state["frac_coords"] - pa("step_corr") * pa("sqrt_sn") * preds[0]) % 1.0, pa("std_corr"))
    _close(lp[2], R._crystal_mean(lc.mean(dim=-1), batch, na), 1e-14, "lp_x = corrector term")
    assert torch.count_nonzero(dl) == 0 and torch.count_nonzero(dt) == 0 and torch.count_nonzero(dxp) == 0
    assert torch.equal(dxc, R.logprobs(s, state, preds)[1][2]) and float(dxc.abs().min()) > 0
    _, _, prior = _case(seed=6)
    v, dv = LR.kl(s, NA, preds, prior, masks)
    assert torch.count_nonzero(v[0]) == 0 and torch.count_nonzero(v[1]) == 0 and float(v[2].min()) > 0
    assert all(torch.count_nonzero(dv[k]) == 0 for k in (0, 1, 3)) and torch.equal(dv[2], R.kl(s, NA, preds, prior)[1][2])


def test_derivatives_are_autograd_of_the_masked_sums_and_zero_where_masked():
    s, state, preds = _case()
    masks = LR.make_masks(NA, "mixed", seed=1)
    kt, kx, kl = masks
    leaves = tuple(p.clone().requires_grad_(True) for p in preds)
    lp, d = LR.logprobs(s, state, leaves, masks)
    g = torch.autograd.grad(sum(v.sum() for v in lp), leaves)           # (px_corr, pl, px_pred, pt)
    for a, b, what in ((d[0], g[1], "dl"), (d[1], g[3], "dt"), (d[2], g[0], "dx_corr"), (d[3], g[2], "dx_pred")):
        _close(a, b, 1e-10, what)
    assert torch.count_nonzero(d[0][kl]) == 0 and torch.count_nonzero(d[1][kt]) == 0 and torch.count_nonzero(d[3][kx]) == 0
    d0 = R.logprobs(s, state, preds)[1]
    assert torch.equal(d[0][~kl], d0[0][~kl]) and torch.equal(d[1][~kt], d0[1][~kt]) and torch.equal(d[3][~kx], d0[3][~kx])
    assert torch.equal(d[2], d0[2])
    _, _, prior = _case(seed=6)
    v, dv = LR.kl(s, NA, leaves, prior, masks)
    gk = torch.autograd.grad(sum(x.sum() for x in v), leaves)
    for a, b, what in ((dv[0], gk[1], "KL dl"), (dv[1], gk[3], "KL dt"), (dv[2], gk[0], "KL dx_corr"), (dv[3], gk[2], "KL dx_pred")):
        _close(a, b, 1e-10, what)


def test_the_fp32_restatement_is_the_same_function():
    """formulas32 / kl32 in float64 agree with logprobs / kl to rounding (the naive 21-image sum against logsumexp); in float32 they stay
    within 1e-3 of max|ref|: a yardstick, not a second definition."""
    s, state, preds = _case()
    _, _, prior = _case(seed=6)
    masks = LR.make_masks(NA, "mixed", seed=1)
    lp, _ = LR.logprobs(s, state, preds, masks)
    v, _ = LR.kl(s, NA, preds, prior, masks)
    s32 = kl_util.step_scalars(*_schedules(), SIGMA_BEGIN, TIMES, STEP_LR, dtype=torch.float32)
    for k, (a, b) in enumerate(zip(LR.formulas32(s, state, preds, masks, torch.float64), lp)):
        _close(a, b, 1e-11, f"float64 formulas, log-prob {k}")
    for k, (a, b) in enumerate(zip(LR.kl32(s, NA, preds, prior, masks, torch.float64), v)):
        _close(a, b, 1e-12, f"float64 formulas, KL {k}")
    for k, (a, b) in enumerate(zip(LR.formulas32(s32, state, preds, masks), lp)):
        assert a.dtype == torch.float32
        _close(a.double(), b, 1e-3, f"float32 formulas, log-prob {k}")
    for k, (a, b) in enumerate(zip(LR.kl32(s32, NA, preds, prior, masks), v)):
        _close(a.double(), b, 1e-3, f"float32 formulas, KL {k}")


# ---- host bookkeeping ---------------------------------------------------------------------------------------------------------------

def _cond(na, seed=3):
    g = torch.Generator().manual_seed(seed)
    B, N = len(na), sum(na)
    return Condition(na, atom_types=torch.randint(1, 101, (N,), generator=g), known_types=torch.rand(N, generator=g) < 0.5,
                     frac_coords=torch.rand(N, 3, generator=g), known_coords=torch.rand(N, generator=g) < 0.5,
                     lattices=torch.randn(B, 3, 3, generator=g), known_lattice=torch.rand(B, generator=g) < 0.5)


FIELDS = ("num_atoms", "atom_types", "known_types", "frac_coords", "known_coords", "lattices", "known_lattice")


def _same(p, q):
    return all(torch.equal(getattr(p, k), getattr(q, k)) for k in FIELDS)


def test_condition_select_against_slicing():
    na = [2, 3, 1, 4, 2]
    c = _cond(na)
    assert _same(c.select(range(5)), c) and _same(c.select([1, 2, 3]), c.slice(1, 4)) and _same(c.select([4]), c.slice(4, 5))
    s = c.select([3, 0, 3])
    assert s.num_atoms.tolist() == [4, 2, 4]
    off = np.cumsum([0] + na)
    rows = list(range(off[3], off[4])) + list(range(off[0], off[1])) + list(range(off[3], off[4]))
    assert torch.equal(s.atom_types, c.atom_types[rows]) and torch.equal(s.known_coords, c.known_coords[rows])
    assert torch.equal(s.frac_coords, c.frac_coords[rows]) and torch.equal(s.lattices, c.lattices[[3, 0, 3]])
    assert torch.equal(s.known_lattice, c.known_lattice[[3, 0, 3]])
    e = c.select([])
    assert len(e) == 0 and e.num_nodes == 0


def test_rollout_select_carries_the_condition():
    from matinvent_amd.sampling import Rollout
    na = torch.tensor([2, 3, 1])
    N, B, Tn = int(na.sum()), len(na), 4
    c = _cond(na.tolist())
    off = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(na, 0)])
    ro = Rollout(torch.randn(Tn + 1, N, 100), torch.rand(Tn + 1, N, 3), torch.rand(Tn + 1, N, 3), torch.randn(Tn + 1, B, 9),
                 torch.randn(Tn + 1, B, 3), na, off, Tn, STEP_LR, c)
    assert ro.select([0, 1, 2]) is ro
    sub = ro.select([2, 0])
    assert sub.num_atoms.tolist() == [1, 2] and _same(sub.condition, c.select([2, 0]))
    assert torch.equal(sub.frac_coords, ro.frac_coords[:, [5, 0, 1]])
    plain = Rollout(ro.atom_types, ro.frac_coords, ro.frac_coords_mid, ro.lattices, ro.lp_old, na, off, Tn, STEP_LR)
    assert plain.condition is None and plain.select([1]).condition is None


def test_header_symbols_and_table():
    from matinvent_amd.build import build
    names = declared_symbols("matinvent_hip_lik.h")
    assert names == ["mi_batch_has_likelihood_mask", "mi_batch_set_likelihood_mask", "mi_traj_read_derivatives"]
    assert sorted(_lib.LIK_SIGNATURES) == names and any(t is _lib.LIK_SIGNATURES for t in _lib.EXTENSION_SIGNATURES)
    lib = ctypes.CDLL(build(verbose=False))
    assert all(hasattr(lib, n) for n in names)
    bound = _lib.load()
    # refused on the host, before any device work: null handles
    assert bound.mi_batch_set_likelihood_mask(None, None, None, None) == _lib.MI_EINVAL and b"null handle" in bound.mi_last_error()
    assert bound.mi_batch_has_likelihood_mask(None) == _lib.MI_EINVAL
    assert bound.mi_traj_read_derivatives(None, None, None, None, None) == _lib.MI_EINVAL


def test_refusals_that_remain_and_the_new_value_errors(tmp_path):
    from matinvent_amd import pipeline, sampling
    from matinvent_amd.diffcsp import DiffCSPModule
    from matinvent_amd.suite import DiffCSPSuite
    c = Condition.composition("NaCl", 2)
    assert check_likelihood("x", None, None) is False and check_likelihood("x", None, c) is False and check_likelihood("x", "free", c) is True
    with pytest.raises(ValueError, match="needs the condition"):
        check_likelihood("x", "free", None)
    with pytest.raises(ValueError, match="neither None nor 'free'"):
        check_likelihood("x", "all", c)
    # without the keyword a condition is refused exactly as before; sample_mdp keeps refusing and has no keyword
    with pytest.raises(ValueError, match="sample_rollout: a condition is not supported"):
        sampling.sample_rollout(2, None, condition=c)
    with pytest.raises(ValueError, match="sample_mdp: a condition is not supported"):
        sampling.sample_mdp(2, None, condition=c)
    with pytest.raises(TypeError):
        sampling.sample_mdp(2, None, condition=c, likelihood="free")
    with pytest.raises(ValueError, match="needs the condition"):
        sampling.sample_rollout(2, None, likelihood="free")
    with pytest.raises(ValueError, match="covers 2 crystals"):
        sampling.sample_rollout(3, None, condition=c, likelihood="free")
    # the module's two entries check the keyword before they touch the device
    m = DiffCSPModule.__new__(DiffCSPModule)
    with pytest.raises(ValueError, match="needs the condition"):
        m.sample(c, likelihood="free")
    with pytest.raises(ValueError, match="needs the condition"):
        m.forward_logprb({}, likelihood="free")
    with pytest.raises(ValueError, match="forward_logprb: a condition is not supported"):
        m.forward_logprb({}, condition=c)
    # MatInventPG: refused without the key, with the old message; accepted with it; a value other than `free` is refused
    suite = DiffCSPSuite("diffcsp", {"batch_size": 4, "num_batches": 1}, {}, device="cpu")
    kw = dict(rl_epoch=1, model_suite=suite, reward=None, finetune_cfg={}, save_dir=str(tmp_path), save_freq=1, device="cpu")
    targets = [{"Na": 1, "Cl": 1}]
    with pytest.raises(ValueError, match="sample_cfg.target_compositions_dict is not supported"):
        pipeline.MatInventPG(sample_cfg={"target_compositions_dict": targets}, **kw)
    with pytest.raises(ValueError, match="sample_cfg.condition is not supported"):
        pipeline.MatInventPG(sample_cfg={"condition": c}, **kw)
    with pytest.raises(ValueError, match="condition_likelihood"):
        pipeline.MatInventPG(sample_cfg={"target_compositions_dict": targets, "condition_likelihood": "all"}, **kw)
    with pytest.raises(ValueError, match="not both"):
        pipeline.MatInventPG(sample_cfg={"target_compositions_dict": targets, "condition": c, "condition_likelihood": "free"}, **kw)


def test_dropin_config_names_the_key_commented_out():
    import os
    from tests.header_util import ROOT
    text = open(os.path.join(ROOT, "dropin", "configs", "pipeline", "mat_invent_pg.yaml")).read()
    lines = [ln for ln in text.splitlines() if "condition_likelihood" in ln]
    assert lines and all(ln.lstrip().startswith("#") for ln in lines)

"""GPU checks of the trajectory likelihood of a conditioned chain (include/matinvent_hip_lik.h) on the 64-wide, 2-layer
network of tests/test_gpu_condition.py with T = 20:

1. the masked log-probabilities, the type head's local derivatives (through type_out.bias's gradient) and the masked KL against the
   float64 restatement tests/lik_ref64.py, zero head weights, at the sizes the kernels loop over;
2. exact properties: an all-false mask is no mask, bit for bit, in all three C entries; masked derivatives are exactly 0.f and free ones
   the unmasked call's bits; taped = untaped; two calls agree;
3. the sampler's record with likelihood="free": same states, same bits where nothing is known, lik_ref64 elsewhere; one stream and split;
4. a conditioned rollout re-evaluated at unchanged weights gives a unit ratio with the mask and does not without it;
5. pg_step on a conditioned rollout, with and without the KL anchor;
6. one MatInventPG loop through dropin/main.py with target_compositions_dict and condition_likelihood: free.

Atom counts of (1): LOOP_NA = [1, 4, 5, 86, 171] -- 5: the first second pass of the four-wave atom loop, 86 and 171: the second and
third pass of the 256-thread coordinate loop (3 n = 258, 513), no count but 4 a multiple of 4; GRID_NA = 300 crystals of one and two
atoms.  Times: 2 and T alternate over the crystals.  Tolerance of (1) and (3): tests/test_gpu_traj_arithmetic._check, imported -- the
device within 4 x the deviation of the float32 formulas (lik_ref64.formulas32 / kl32 on the CPU, same inputs) from float64, relative to
max|ref|, at least 4 * 2^-24.  MI_TOL_REPORT=1 prints the figures."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tests.test_gpu_condition as CT
import tests.test_gpu_pg_prior_kl as KLT
import tests.test_gpu_policy_gradient as PG
import tests.test_gpu_respaced_chain as RC
import tests.test_gpu_traj_arithmetic as TA
from matinvent_amd import _lib, policy
from matinvent_amd.conditioning import Condition
from matinvent_amd.cspnet import _ptr, _stream
from matinvent_amd.sampling import Rollout
from matinvent_amd.structure import reduced_formula
from oracle import diffcsp_oracle as O
from tests import kl_util, lik_ref64 as LR, traj_ref64 as R
from tests.gpu_util import Box, make_module

pytestmark = pytest.mark.gpu

T = 20
STEP_LR = RC.STEP_LR
SIGMA_BEGIN = 0.005
EPS = PG.EPS
LOOP_NA = [1, 4, 5, 86, 171]
GRID_NA = [1, 2] * 150
LP = TA.LP
STATE = CT.STATE
W = (0.5, 1.0, 2.0)


def test_the_shapes_reach_what_they_are_chosen_for():
    assert [3 * n for n in LOOP_NA if 3 * n > 256] == [258, 513] and 5 in LOOP_NA and 4 in LOOP_NA and 1 in LOOP_NA
    assert len(GRID_NA) == 300 and set(GRID_NA) == {1, 2}
    for mode in ("mixed",):
        kt, kx, kl = LR.make_masks(LOOP_NA, mode, seed=1)
        assert kt.any() and (~kt).any() and kx.any() and (~kx).any() and kl.any() and (~kl).any() and not torch.equal(kt, kx)


# ---- helpers ------------------------------------------------------------------------------------------------------------------------

def _module(P):
    return make_module(64, 2, 8, T, P, sigmas_norm=torch.cat([torch.ones(1), torch.linspace(0.6, 1.4, T)]))


def _zero_head_params(seed):
    P = O.init_params(RC.HP, seed=seed, head_scale=0.1)
    for k in TA.HEADS:
        P["decoder." + k] = torch.zeros_like(P["decoder." + k])
    P["decoder.type_out.bias"] = torch.randn(100, generator=torch.Generator().manual_seed(seed + 1000))
    return P


def _condition(na, masks):
    """A Condition that carries `masks` (its clean values are never read by the likelihood mask)."""
    kt, kx, kl = masks
    N, B = sum(na), len(na)
    return Condition(na, atom_types=torch.ones(N, dtype=torch.long), known_types=kt, frac_coords=torch.zeros(N, 3), known_coords=kx,
                     lattices=torch.zeros(B, 3, 3), known_lattice=kl)


def _times(B):
    return torch.tensor([2, T] * (B // 2) + [T] * (B % 2))


def _rollout(na, state, t, seed, cond=None):
    """A hand-built Rollout of T steps: uniform noise everywhere, crystal b's `state` written at t[b] and t[b] - 1."""
    na_t = torch.tensor(na)
    B, N = len(na), sum(na)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *shape: torch.rand(*shape, device="cuda", generator=gen)
    ro = Rollout(r(T + 1, N, 100), r(T + 1, N, 3), r(T + 1, N, 3), r(T + 1, B, 9), r(T + 1, B, 3), na_t.clone(),
                 torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(na_t, 0)]), T, STEP_LR, cond)
    an, ab = torch.arange(N, device="cuda"), torch.arange(B, device="cuda")
    tn, tb = torch.repeat_interleave(t, na_t).cuda(), t.cuda()
    ro.atom_types[tn, an], ro.atom_types[tn - 1, an] = state["atom_types"].cuda(), state["next_atom_types"].cuda()
    ro.frac_coords[tn, an], ro.frac_coords[tn - 1, an] = state["frac_coords"].cuda(), state["next_frac_coords"].cuda()
    ro.frac_coords_mid[tn, an] = state["frac_coords_mid"].cuda()
    ro.lattices[tb, ab], ro.lattices[tb - 1, ab] = state["lattices"].view(-1, 9).cuda(), state["next_lattices"].view(-1, 9).cuda()
    return ro


def _handles(m, na, cond, n=2):
    hs = tuple(m.make_batch(na) for _ in range(n))
    if cond is not None:
        for h in hs:
            cond.attach_likelihood(m, h)
            assert _lib.load().mi_batch_has_likelihood_mask(h._h) == 1
    return hs


def _derivatives(handle):
    """(dl [B, 9], dx [N, 3], dt [N, 100]) the last taped call left on `handle`."""
    B, N = handle.num_graphs, handle.num_nodes
    dl, dx, dt = torch.empty(B, 9, device="cuda"), torch.empty(N, 3, device="cuda"), torch.empty(N, 100, device="cuda")
    _lib.check(_lib.load().mi_traj_read_derivatives(handle._h, _ptr(dl), _ptr(dx), _ptr(dt), _stream()), "mi_traj_read_derivatives")
    torch.cuda.synchronize()
    return dl, dx, dt


def _pair(m, na):
    return m.__dict__["_traj_cache"][tuple(int(v) for v in na)].handles


def _collect(checks):
    bad = []
    for args in checks:
        try:
            TA._check(*args)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)


# ---- 1. against float64 -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(shape):
    """Zero heads, one written state per shape, the step scalars in both precisions: computed once, shared, left unchanged."""
    na = LOOP_NA if shape == "loop" else GRID_NA
    P, Pp = _zero_head_params(3), _zero_head_params(4)
    c = SimpleNamespace(na=na, B=len(na), N=sum(na), bias=P["decoder.type_out.bias"], bias_p=Pp["decoder.type_out.bias"], m=_module(P),
                        prior=_module(Pp))
    c.batch = torch.repeat_interleave(torch.arange(c.B), torch.tensor(na))
    c.t = _times(c.B)
    beta, sigma = TA._schedules(c.m)
    c.s = R.step_scalars(beta, sigma, SIGMA_BEGIN, c.t, STEP_LR)
    c.s32 = kl_util.step_scalars(beta, sigma, SIGMA_BEGIN, c.t, STEP_LR, dtype=torch.float32)
    c.state = R.build_state(na, c.t, c.s, dict(pred_t=c.bias), seed=7)
    c.preds, c.preds_p = R.zero_head_preds(na, c.bias), R.zero_head_preds(na, c.bias_p)
    return c


@pytest.mark.parametrize("mode", ["all", "none", "mixed"])
@pytest.mark.parametrize("shape", ["loop", "grid"])
def test_zero_heads_masked_logprobs_gradient_and_kl_vs_float64(shape, mode):
    c = _case(shape)
    assert {2, T} <= set(c.t.tolist())
    masks = LR.make_masks(c.na, mode, seed=1)
    cond = _condition(c.na, masks)
    lp64, d64 = LR.logprobs(c.s, R.to64(c.state), c.preds, masks)
    pt32 = c.bias[None, :].expand(c.N, 100).clone().requires_grad_(True)
    p32 = (torch.zeros(c.N, 3), torch.zeros(c.B, 3, 3), torch.zeros(c.N, 3), pt32)
    out32 = LR.formulas32(c.s32, c.state, p32, masks)
    # the three log-probabilities, untaped and taped
    with torch.no_grad():
        plain = c.m.forward_logprb(dict(c.state), step_lr=STEP_LR, condition=cond, likelihood="free")
    c.m.decoder.theta.grad = None
    taped = c.m.forward_logprb(dict(c.state), step_lr=STEP_LR, condition=cond, likelihood="free")
    assert taped[0].requires_grad and not plain[0].requires_grad
    checks = []
    for k in range(3):
        assert torch.equal(plain[k], taped[k].detach()), LP[k]
        checks.append((plain[k], lp64[k], out32[k].detach(), f"{shape} {mode} {LP[k]}"))
    if mode == "all":   # hand values: nothing of the predictor is left
        assert torch.count_nonzero(plain[0]) == 0 and torch.count_nonzero(plain[1]) == 0
    # the type head's local derivatives through type_out.bias's gradient; the trunk's gradient is exactly zero
    g = [torch.randn(c.B, generator=torch.Generator().manual_seed(12 + k)) for k in range(3)]
    sum((g[k].cuda() * taped[k]).sum() for k in range(3)).backward()
    dev_bias = TA._grads(c.m)["type_out.bias"].clone()
    TA._assert_trunk_gradient_is_zero(c.m, c.m.decoder.theta.grad)
    c.m.decoder.theta.grad = None
    bias64 = (g[1].double()[c.batch][:, None] * d64[1]).sum(dim=0)
    bias32 = torch.autograd.grad(sum((g[k] * out32[k]).sum() for k in range(3)), pt32)[0].sum(dim=0)
    if mode == "all":
        assert torch.count_nonzero(dev_bias) == 0 and torch.count_nonzero(bias64) == 0
    else:
        assert float(bias64.abs().max()) > 0
        checks.append((dev_bias, bias64, bias32, f"{shape} {mode} grad type_out.bias vs sum of masked seeds"))
    # the masked KL: both networks with zero heads and different biases -- KL_l = KL_x = 0, KL_t over the free atoms
    ro = _rollout(c.na, c.state, c.t, seed=3, cond=cond)
    M, beta_kl = 2 * c.B, 0.7
    hs = _handles(c.m, c.na, cond)
    hp, = _handles(c.prior, c.na, cond, n=1)
    grad, stats, lp, kl_dev = KLT._kl_step(c.m, c.prior, ro, c.t.numpy(), torch.zeros(c.B, device="cuda"), EPS, W, M, beta_kl, handles=hs,
                                           prior_handle=hp)
    for k in range(3):
        assert torch.equal(lp[k], plain[k]), ("fused", LP[k])
    assert torch.count_nonzero(kl_dev[0]) == 0 and torch.count_nonzero(kl_dev[2]) == 0
    val, dk = LR.kl(c.s, c.na, c.preds, c.preds_p, masks)
    pa32 = tuple(v.float() for v in c.preds[:3]) + (c.bias[None, :].expand(c.N, 100).clone().requires_grad_(True),)
    v32 = LR.kl32(c.s32, c.na, pa32, c.preds_p, masks)
    coef = beta_kl * W[1] / M
    kb32 = torch.autograd.grad((coef * v32[1]).sum(), pa32[3])[0].sum(dim=0)
    dev_kb = TA._grads(c.m, grad)["type_out.bias"]
    if mode == "all":
        assert torch.count_nonzero(kl_dev[1]) == 0 and torch.count_nonzero(stats[4]) == 0 and torch.count_nonzero(dev_kb) == 0
    else:
        assert float(val[1].abs().max()) > 0
        checks += [(kl_dev[1], val[1], v32[1].detach(), f"{shape} {mode} KL_t"),
                   (stats[4], W[1] * val[1], W[1] * v32[1].detach(), f"{shape} {mode} statistics row 4"),
                   (dev_kb, coef * dk[1].sum(dim=0), kb32, f"{shape} {mode} KL grad type_out.bias")]
    TA._assert_trunk_gradient_is_zero(c.m, grad)
    _collect(checks)


# ---- 2. exact properties ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def base():
    return RC._base()[0]


@pytest.fixture(scope="module")
def written():
    """A written state at na = [1, 4, 5, 12] for the module of `base` (non-zero heads: every term finite, every derivative non-zero)."""
    na, t = [1, 4, 5, 12], torch.tensor([2, T, 11, T])
    m = RC._base()[0]
    s = R.step_scalars(*TA._schedules(m), SIGMA_BEGIN, t, STEP_LR)
    return SimpleNamespace(na=na, t=t, B=len(na), N=sum(na), state=R.build_state(na, t, s, dict(pred_t=torch.zeros(100)), seed=21))


def _taped(m, w, cond):
    """One taped forward_logprb + backward with fixed upstream gradients: (log-probs, theta.grad, (dl, dx_pred, dt), dx_corr)."""
    m.decoder.theta.grad = None
    kw = {} if cond is None else dict(condition=cond, likelihood="free")
    out = m.forward_logprb(dict(w.state), step_lr=STEP_LR, **kw)
    bc, bp = _pair(m, w.na)
    assert _lib.load().mi_batch_has_likelihood_mask(bp._h) == 0          # the pair carries the mask for the call alone
    dl, dxp, dt = _derivatives(bp)
    dxc = _derivatives(bc)[1]
    g = [torch.randn(w.B, generator=torch.Generator().manual_seed(5 + k)).cuda() for k in range(3)]
    sum((g[k] * out[k]).sum() for k in range(3)).backward()
    grad = m.decoder.theta.grad.clone()
    m.decoder.theta.grad = None
    return [v.detach().clone() for v in out[:3]], grad, (dl, dxp, dt), dxc


def test_all_false_mask_is_no_mask_and_masked_derivatives_are_exact_zeros(base, written):
    w = written
    none = _condition(w.na, LR.make_masks(w.na, "none"))
    masks = LR.make_masks(w.na, "mixed", seed=2)
    kt, kx, kl = (v.cuda() for v in masks)
    mixed = _condition(w.na, masks)
    lp0, g0, (dl0, dxp0, dt0), dxc0 = _taped(base, w, None)
    assert all(bool(torch.isfinite(v).all()) for v in lp0) and float(g0.abs().max()) > 0
    lp1, g1, (dl1, dxp1, dt1), dxc1 = _taped(base, w, none)
    for a, b in zip(lp0 + [g0, dl0, dxp0, dt0, dxc0], lp1 + [g1, dl1, dxp1, dt1, dxc1]):
        assert torch.equal(a, b)
    lp2, g2, (dl2, dxp2, dt2), dxc2 = _taped(base, w, mixed)
    assert torch.count_nonzero(dl2[kl]) == 0 and torch.count_nonzero(dt2[kt]) == 0 and torch.count_nonzero(dxp2[kx]) == 0
    for v in (dl2[kl], dt2[kt], dxp2[kx]):
        assert not bool(torch.signbit(v).any())                            # 0.f, not -0.f
    assert torch.equal(dl2[~kl], dl0[~kl]) and torch.equal(dt2[~kt], dt0[~kt]) and torch.equal(dxp2[~kx], dxp0[~kx])
    assert torch.equal(dxc2, dxc0)
    assert float(dl0[kl].abs().min()) > 0 and float(dt0[kt].abs().min()) > 0 and float(dxp0[kx].abs().min()) > 0
    assert not torch.equal(g2, g0) and not any(torch.equal(a, b) for a, b in zip(lp2, lp0))
    # two identical calls are bit-identical (taped against untaped is asserted where the predictions do not depend on the evaluation's form:
    # with zero heads, in test_zero_heads_masked_logprobs_gradient_and_kl_vs_float64 -- a training and an inference evaluation of a network
    # with non-zero heads differ by rounding, as without a mask)
    lp3, g3, d3, dxc3 = _taped(base, w, mixed)
    for k in range(3):
        assert torch.equal(lp3[k], lp2[k])
    assert torch.equal(g3, g2) and all(torch.equal(a, b) for a, b in zip(d3, (dl2, dxp2, dt2))) and torch.equal(dxc3, dxc2)


@pytest.mark.parametrize("with_kl", [False, True])
def test_all_false_mask_gives_the_bits_of_no_mask_in_the_micro_steps(base, written, with_kl):
    w = written
    none = _condition(w.na, LR.make_masks(w.na, "none"))
    mixed = _condition(w.na, LR.make_masks(w.na, "mixed", seed=2))
    ro = _rollout(w.na, w.state, w.t, seed=5)
    A = torch.tensor([1.0, -0.7, 0.4, -1.3], device="cuda")
    prior = make_module(64, 2, 8, T, KLT._perturbed(RC._base()[1], seed=77), sigmas_norm=base.sigma_scheduler.sigmas_norm.cpu())

    def step(cond):
        hs = _handles(base, w.na, cond)
        if with_kl:
            hp, = _handles(prior, w.na, cond, n=1)
            return KLT._kl_step(base, prior, ro, w.t.numpy(), A, 0.2, W, w.B, 0.3, handles=hs, prior_handle=hp)
        return PG._fused(base, ro, w.t.numpy(), A, 0.2, W, w.B, hs)

    ref, same, masked, again = step(None), step(none), step(mixed), step(mixed)
    for a, b in zip(ref, same):
        assert torch.equal(a, b)
    for a, b in zip(masked, again):
        assert torch.equal(a, b)
    assert not torch.equal(masked[0], ref[0]) and not torch.equal(masked[2], ref[2])
    assert all(bool(torch.isfinite(v).all()) for v in masked)


def test_handles_of_a_call_must_carry_the_same_mask(base, written):
    w = written
    mixed = _condition(w.na, LR.make_masks(w.na, "mixed", seed=2))
    other = _condition(w.na, LR.make_masks(w.na, "mixed", seed=3))
    ro = _rollout(w.na, w.state, w.t, seed=5)
    A = torch.ones(w.B, device="cuda")
    hs = _handles(base, w.na, mixed)
    Condition.clear_likelihood(hs[0])
    with pytest.raises(_lib.MIError, match="likelihood mask") as e:
        PG._fused(base, ro, w.t.numpy(), A, 0.2, W, w.B, hs)
    assert e.value.code == _lib.MI_EINVAL
    other.attach_likelihood(base, hs[0])
    with pytest.raises(_lib.MIError, match="likelihood mask"):
        PG._fused(base, ro, w.t.numpy(), A, 0.2, W, w.B, hs)
    mixed.attach_likelihood(base, hs[0])
    hp, = _handles(base, w.na, None, n=1)
    with pytest.raises(_lib.MIError, match="prior's batch handle carries another likelihood mask"):
        KLT._kl_step(base, base, ro, w.t.numpy(), A, 0.2, W, w.B, 0.3, handles=hs, prior_handle=hp)
    # a value other than 0 / 1 is refused and the handle keeps what it had
    bad = np.zeros(w.N, dtype=np.int32)
    bad[3] = 2
    import ctypes as C
    rc = _lib.load().mi_batch_set_likelihood_mask(hs[0]._h, bad.ctypes.data_as(C.POINTER(C.c_int)), None, None)
    assert rc == _lib.MI_EINVAL and _lib.load().mi_batch_has_likelihood_mask(hs[0]._h) == 1
    PG._fused(base, ro, w.t.numpy(), A, 0.2, W, w.B, hs)                  # still the pair's common mask


# ---- 3. the sampler's record --------------------------------------------------------------------------------------------------------

def _chain_condition():
    """Six crystals: 0, 1, 2 and 5 mixed, 3 with nothing known, 4 with everything known."""
    na = RC.NA + RC.NA[::-1]                                               # [1, 3, 7, 7, 3, 1]
    c = CT._cond(na, seed=32)
    off = np.cumsum([0] + na)
    for k in (c.known_types, c.known_coords):
        k[off[3]:off[4]], k[off[4]:off[5]] = False, True
    c.known_lattice[3], c.known_lattice[4] = False, True
    c.known_types[off[2]], c.known_types[off[2] + 1] = True, False          # the 7-atom crystal: mixed in both parts
    c.known_coords[off[2]], c.known_coords[off[2] + 1] = False, True
    return na, c


def _device_predictions(v, cur, nxt, na, t):
    """The device's own predictions of step t: (px_corr, pl, px_pred, pt), float64, from two untaped forward_logprb calls whose corrector
    and predictor inputs coincide (at x_t, then at x_mid)."""
    st = dict(atom_types=cur["atom_types"], lattices=cur["lattices"], next_atom_types=nxt["atom_types"], next_frac_coords=nxt["frac_coords"],
              next_lattices=nxt["lattices"], num_atoms=torch.tensor(na), timesteps=torch.full((len(na),), t))
    with torch.no_grad():
        _, pxc, _ = v.forward_logprb(dict(st, frac_coords=cur["frac_coords"], frac_coords_mid=cur["frac_coords"]), step_lr=STEP_LR)[3]
        pl, pxp, pt = v.forward_logprb(dict(st, frac_coords=cur["frac_coords_mid"], frac_coords_mid=cur["frac_coords_mid"]), step_lr=STEP_LR)[3]
    return tuple(x.double().cpu() for x in (pxc, pl, pxp, pt))


@pytest.mark.parametrize("S", [None, 5])
def test_recorded_logprobs_of_a_conditioned_chain(base, S):
    v = base if S is None else base.respaced(S)
    Tv = v.beta_scheduler.timesteps
    na, c = _chain_condition()
    masks = LR.masks_of(c)
    kw = dict(step_lr=STEP_LR, seed=43, record=True, condition=c)
    plain = v.sample(Box(na), streams=1, **kw)
    lik = v.sample(Box(na), streams=1, likelihood="free", **kw)
    assert sorted(lik[1]) == list(range(Tv + 1))
    for k in STATE:
        assert torch.equal(lik[0][k], plain[0][k]), k
    batch = torch.repeat_interleave(torch.arange(len(na)), torch.tensor(na))
    count = lambda known: torch.zeros(len(na)).index_add(0, batch, known.float())
    none_t, none_x = count(c.known_types) == 0, count(c.known_coords) == 0
    free = dict(log_prob_l=~c.known_lattice, log_prob_t=none_t, log_prob_x=none_x)
    assert all(bool(f.any()) and not bool(f.all()) for f in free.values())
    beta, sigma = TA._schedules(v)
    checks = []
    for t in range(Tv, 1, -1):
        cur, nxt = lik[1][t], lik[1][t - 1]
        for k in STATE + ("frac_coords_mid",):
            assert torch.equal(cur[k], plain[1][t][k]), (t, k)
        for k in LP:
            assert torch.equal(cur[k][free[k].cuda()], plain[1][t][k][free[k].cuda()]), (t, k)
        assert not torch.equal(cur["log_prob_t"], plain[1][t]["log_prob_t"])
        assert float(cur["log_prob_l"][4]) == 0.0 and float(cur["log_prob_t"][4]) == 0.0
        if t not in (Tv, Tv // 2, 2):
            continue
        tt = torch.full((len(na),), t)
        s = R.step_scalars(beta, sigma, SIGMA_BEGIN, tt, STEP_LR)
        s32 = kl_util.step_scalars(beta, sigma, SIGMA_BEGIN, tt, STEP_LR, dtype=torch.float32)
        preds = _device_predictions(v, cur, nxt, na, t)
        st = dict(atom_types=cur["atom_types"], frac_coords=cur["frac_coords"], frac_coords_mid=cur["frac_coords_mid"], lattices=cur["lattices"],
                  next_atom_types=nxt["atom_types"], next_frac_coords=nxt["frac_coords"], next_lattices=nxt["lattices"])
        st = {k: x.cpu() for k, x in st.items()}
        st["num_atoms"] = torch.tensor(na)
        ref, _ = LR.logprobs(s, R.to64(st), preds, masks)
        r32 = LR.formulas32(s32, st, preds, masks)
        for i, k in enumerate(LP):
            checks.append((cur[k], ref[i], r32[i], f"S = {S}, t = {t}, recorded {k}"))
    _collect(checks)
    # a split batch: the same states as the split call without the keyword, bit for bit; against one stream the tolerances of
    # tests/test_gpu_condition.py for split against unsplit
    two_plain = v.sample(Box(na), streams=2, **kw)
    two = v.sample(Box(na), streams=2, likelihood="free", **kw)
    for t in two[1]:
        for k in two[1][t]:
            if k in LP:
                f = free[k].cuda()
                assert torch.equal(two[1][t][k][f], two_plain[1][t][k][f]), (t, k)
                np.testing.assert_allclose(two[1][t][k].cpu().numpy(), lik[1][t][k].cpu().numpy(), rtol=2e-4, atol=2e-4, err_msg=f"{t} {k}")
            elif k not in ("num_atoms", "batch_idx"):
                assert torch.equal(two[1][t][k], two_plain[1][t][k]), (t, k)

# ---- 4. unit ratio ------------------------------------------------------------------------------------------------------------------

def _conditions():
    from matinvent_amd.data import CrystalData
    comp = Condition.composition([{"Li": 2, "O": 1}, {"Na": 1, "Cl": 1}], 6)
    crystal = CrystalData(torch.tensor([[0.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.25, 0.75, 0.5], [0.7, 0.2, 0.9], [0.1, 0.6, 0.3]]),
                          torch.tensor([3, 3, 8, 11, 17]), torch.tensor([[4.2, 5.1, 6.3]]), torch.tensor([[90.0, 95.0, 100.0]]))
    tmpl = Condition.template(crystal, 6, types=True, coords=[True, False, True, False, False], lattice=True)
    return dict(composition=comp, template=tmpl)


def _conditioned_rollout(m, cond, seed):
    from matinvent_amd import sampling
    data, ro = sampling.sample_rollout(len(cond), m, step_lr=STEP_LR, seed=seed, geometric_filter=False, condition=cond, likelihood="free")
    assert ro.condition is not None and ro.num_atoms.tolist() == cond.num_atoms.tolist() and len(data) == len(cond)
    return data, ro


@pytest.mark.parametrize("kind", ["composition", "template"])
def test_conditioned_rollout_at_unchanged_weights_gives_unit_ratio_only_with_the_mask(kind):
    """test_gpu_policy_gradient.test_old_logprobs_at_unchanged_weights_give_unit_ratio's bound, formula and constants copied:
    |log rho| <= sum_k w_k (1e-4 + 1e-4 |lp_k|), at t = T, T / 2 and 2.  The same rollout without the mask must break it."""
    m = make_module(64, 2, 8, T, O.init_params(RC.HP, seed=4, head_scale=0.1))
    cond = _conditions()[kind]
    data, ro = _conditioned_rollout(m, cond, seed=11)
    assert [reduced_formula(d.atom_types.tolist()) for d in data] == [reduced_formula(cond.atom_types[a:b].tolist())
                                                                      for a, b in zip(ro.node_offsets[:-1], ro.node_offsets[1:])]
    B = ro.num_graphs
    na = [int(v) for v in ro.num_atoms]
    masked, bare = _handles(m, na, ro.condition), _handles(m, na, None)
    w = (0.5, 1.0, 2.0)
    broken = 0
    for t in (T, T // 2, 2):
        lpk = ro.lp_old[t].abs()
        bound = sum(w[k] * (1e-4 + 1e-4 * lpk[:, k]) for k in range(3))
        _, stats, _ = PG._fused(m, ro, np.full(B, t), torch.ones(B, device="cuda"), 1e-4, w, B, masked)
        logr = stats[1].log().abs()
        assert bool((logr <= bound).all()), (t, logr.tolist(), bound.tolist())
        _, stats, _ = PG._fused(m, ro, np.full(B, t), torch.ones(B, device="cuda"), 1e-4, w, B, bare)
        broken += int((~(stats[1].log().abs() <= bound)).sum())
    assert broken >= 1


# ---- 5. pg_step ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kl_coef", [0.0, 0.05])
def test_pg_step_on_a_conditioned_rollout(kl_coef):
    P = O.init_params(RC.HP, seed=9, head_scale=0.1)
    Pp = KLT._perturbed(P, seed=77, scale=0.05)
    cond = _conditions()["template"]
    m0 = make_module(64, 2, 8, T, P)
    _, ro = _conditioned_rollout(m0, cond, seed=41)
    B = ro.num_graphs
    rewards = np.array([0.2, 0.9, 0.5, 0.1, 0.6, 0.4])
    cfg = dict(lr=1e-4, epochs=2, timesteps=5, accum_steps=2, clip_range=0.2, adv_clip=5.0, logprob_weights=[1.0, 1.0, 1.0], kl_coef=kl_coef)
    runs = []
    for _ in range(2):
        m, prior = make_module(64, 2, 8, T, P), make_module(64, 2, 8, T, Pp)
        stats = policy.pg_step(m, ro, rewards, cfg, seed=123, log=lambda s: None, prior=prior if kl_coef else None)
        assert len(stats) == 2 and all(np.isfinite(list(s.values())).all() for s in stats)
        assert ("prior_kl" in stats[0]) == (kl_coef > 0)
        runs.append(m.decoder.theta.detach().clone())
    assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0], m0.decoder.theta.detach())
    # one micro-step: the masked gradient is not the unmasked one; with everything known but the coordinates the lattice and type heads get none
    prior = make_module(64, 2, 8, T, Pp)
    na = [int(v) for v in ro.num_atoms]
    t = np.array([T, 2, 7, 11, T, 2])
    A = torch.from_numpy(policy.advantages(rewards)).cuda()

    def grad(c):
        hs = _handles(m0, na, c)
        if kl_coef:
            hp, = _handles(prior, na, c, n=1)
            return KLT._kl_step(m0, prior, ro, t, A, 0.2, W, B, kl_coef, handles=hs, prior_handle=hp)[0]
        return PG._fused(m0, ro, t, A, 0.2, W, B, hs)[0]

    g_masked, g_bare = grad(ro.condition), grad(None)
    assert bool(torch.isfinite(g_masked).all()) and not torch.equal(g_masked, g_bare)
    N = sum(na)
    coords_free = _condition(na, (torch.ones(N, dtype=torch.bool), torch.zeros(N, dtype=torch.bool), torch.ones(B, dtype=torch.bool)))
    g = PG._per_tensor(m0, grad(coords_free))
    heads = [k for k in g if k.startswith(("lattice_out.", "type_out."))]
    assert "lattice_out.weight" in heads and "type_out.weight" in heads
    for k in heads:
        assert torch.count_nonzero(g[k]) == 0, k
    assert float(g["coord_out.weight"].abs().max()) > 0
    for k in ("lattice_out.weight", "type_out.weight"):
        assert float(PG._per_tensor(m0, g_bare)[k].abs().max()) > 0, k


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------

def test_dropin_pg_pipeline_with_target_compositions(tmp_path, monkeypatch):
    """pipeline=mat_invent_pg through dropin/main.py with sample_cfg.target_compositions_dict and condition_likelihood: free (and
    sample_steps = 5: rollout and training run on a view): every sampled crystal has one of the formulas, pg_step sees the condition of
    the kept crystals, the epoch dicts are finite and the agent moved.  Without the key the loop is refused as before."""
    from matinvent_amd import sampling
    seen, sampled = [], []
    real_pg, real_ro = policy.pg_step, sampling.sample_rollout

    def spy_pg(agent, rollout, rewards, cfg, **kw):
        out = real_pg(agent, rollout, rewards, cfg, **kw)
        seen.append((rollout, out))
        return out

    def spy_ro(*a, **kw):
        out = real_ro(*a, **kw)
        sampled.extend(out[0])
        return out

    monkeypatch.setattr(policy, "pg_step", spy_pg)
    monkeypatch.setattr(sampling, "sample_rollout", spy_ro)
    args = ["pipeline=mat_invent_pg", "pipeline.finetune_cfg.timesteps=4", "pipeline.finetune_cfg.accum_steps=2", "pipeline.finetune_cfg.epochs=1",
            "pipeline.finetune_cfg.kl_coef=0.01", "+sample_cfg.target_compositions_dict=[{Li: 2, O: 1}, {Na: 1, Cl: 1}]"]
    rl = RC._run_dropin(tmp_path, ["expname=pgc", "+sample_cfg.condition_likelihood=free"] + args)
    assert len(sampled) == 4 and [reduced_formula(d.atom_types.tolist()) for d in sampled] == CT.FORMULAS * 2
    assert len(seen) == 1
    rollout, epochs = seen[0]
    assert rollout.T == 5 and rollout.condition is not None and rollout.condition.num_atoms.tolist() == rollout.num_atoms.tolist()
    assert bool(rollout.condition.known_types.all()) and not bool(rollout.condition.known_coords.any())
    assert epochs and all(np.isfinite(list(e.values())).all() for e in epochs)
    rows = (tmp_path / "exp_res" / "pgc" / "metrics.csv").read_text().strip().splitlines()
    assert len(rows) == 2 and "prior_kl" in rows[0]
    d = (rl.agent.decoder.theta - rl.prior.decoder.theta).abs().max().item()
    assert 0 < d < 1e-2
    with pytest.raises(ValueError, match="sample_cfg.target_compositions_dict is not supported"):
        RC._run_dropin(tmp_path, ["expname=pgr"] + args)

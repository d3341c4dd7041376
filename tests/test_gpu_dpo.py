"""GPU checks of the preference (Diffusion-DPO) fine-tune (matinvent_amd/csrc/dpo.hip under backward.hip's micro-step driver,
matinvent_amd.preference, pipeline.MatInventDPO) against the float64 reference tests/dpo_ref64.py.

Method, sets and network are tests/test_gpu_ft_arithmetic.py's (imported, not copied): with the head weight matrices of agent and prior
zero, both predict exactly pl = 0, px = 0, pt = their own type_out.bias, so d_b, m_p, the statistics rows and the type_out.bias gradient are
closed forms of the set, the noise and the two biases -- the float64 reference IS fed the device's predictions -- every trunk gradient is
exactly zero and the head weights' gradients are seeds^T h.  LOOP_NA = [1, 2, 85, 86, 3, 171]: one, two and three trips of the 256-thread
loops; GRID_NA: 300 crystals.

Tolerances (DESIGN 30's rule, computed here): the yardstick of a quantity is the deviation of the same formulas evaluated in float32 on
the CPU from float64, relative to max|ref64|; the device gets 4 times that, never less than 4 * 2^-24.  Device noise: plus the first-order
bound of what the Philox draws' libm round-off (atol 5e-6) can move.  MI_TOL_REPORT=1 prints yardstick, device error and tolerance."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import tests.test_gpu_ft_arithmetic as FA
import tests.test_gpu_traj_arithmetic as TA
from oracle import diffcsp_oracle as O
from tests import dpo_ref64 as D
from tests import ft_ref64 as R
from tests.gpu_util import make_module

pytestmark = pytest.mark.gpu

T, ACCUM = FA.T, FA.ACCUM
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# crystal 0 wins twice, crystal 1 wins once and loses once, crystal 4 sits in no pair
LOOP_PAIRS = [(0, 1), (0, 2), (1, 3), (5, 2), (3, 5)]
# 600 pairs over 300 crystals: crystal 0 is the winner of the first 300 (its slot list takes two trips of the 256-thread loop)
GRID_PAIRS = [(0, 1 + k % 299) for k in range(300)] + [(1 + k % 299, 1 + (7 * k + 3) % 299) for k in range(300)]
GRID_PAIRS = [(w, l if l != w else (l % 299) + 1) for w, l in GRID_PAIRS]
HEADS_PAIRS = [(0, 1), (2, 1), (0, 2)]
HEADS_T = 100
BETA = 0.5
NAMES = ["decoder." + k for k in FA.HEADS + ("type_out.bias",)]


def test_the_pair_lists_reach_what_they_are_chosen_for():
    """Arithmetic facts of the pair lists (no device work)."""
    w, l = [p[0] for p in LOOP_PAIRS], [p[1] for p in LOOP_PAIRS]
    assert w.count(0) == 2 and w.count(1) == 1 and l.count(1) == 1 and 4 not in w + l and all(a != b for a, b in LOOP_PAIRS)
    assert len(GRID_PAIRS) == 600 and sum(1 for p in GRID_PAIRS if p[0] == 0) == 300 and all(a != b for a, b in GRID_PAIRS)
    assert max(max(p) for p in GRID_PAIRS) < len(FA.GRID_NA) and len(FA.GRID_NA) > 256


# ---- helpers ------------------------------------------------------------------------------------------------------------------------

def _handle(c):
    from matinvent_amd import finetune
    return c.m._batch_for(finetune._host_atoms(c.batch))


def _dpo_micro(c, idx, nz, pairs, beta, grad, stats, p_global, call_id=1):
    """mi_dpo_micro_step through preference._dpo_micro_step with real out_delta / out_margin buffers; returns them."""
    from matinvent_amd import preference
    torch.cuda.synchronize()
    _handle(c).set_pairs(pairs)
    delta = torch.full((c.B,), float("nan"), device="cuda")
    margin = torch.full((len(pairs),), float("nan"), device="cuda")
    preference._dpo_micro_step(c.m, c.prior, c.batch, idx, nz, beta, p_global, ACCUM, grad, stats, delta, margin, call_id=call_id)
    torch.cuda.synchronize()
    return delta, margin


def _closed_form(c, idx, nz, pairs, beta, p_global, dtype=torch.float64):
    """One zero-head micro-step at time index idx from the closed-form predictions: dpo_ref64.micro_step's dict + `bias` (the type_out.bias
    gradient, sum_i seed_t[i, :])."""
    out = R.add_noise(c.fs, R.schedule(c.tables, [T - idx] * c.B), nz)
    pa, pp, tg = R.zero_head_preds(c.na, c.bias_a), R.zero_head_preds(c.na, c.bias_p), (out["rand_l"], out["tar_x"], out["rand_t"])
    ms = D.micro_step(pa, pp, tg, R.COSTS, c.na, pairs, beta, p_global, ACCUM, dtype)
    ms["bias"] = ms["seeds"][2].sum(dim=0)
    return ms


def _oracle(c, idx, nz, dtype, pairs, beta, p_global):
    return D.oracle_dpo_micro_step(c.hp, c.P, c.Q, c.tables, c.fs, nz, dtype, pairs, beta, idx, p_global, accum=ACCUM, freqs=c.freqs, grad=True)


def _zero_head_steps(c, idxs, pairs, beta, p_global, what, seeds=(40, 41)):
    """len(idxs) micro-steps into one gradient and one statistics buffer; every output against the references.  Returns (grad, stats, the
    per-step (delta, margin))."""
    FA._offsets(c)
    grad, stats = torch.zeros_like(c.m.decoder.theta), torch.zeros(3, device="cuda")
    checks, tot, outs = [], None, []
    for k, idx in enumerate(idxs):
        nz = R.noise(c.fs, seed=seeds[k])
        delta, margin = _dpo_micro(c, idx, nz, pairs, beta, grad, stats, p_global)
        outs.append((delta.clone(), margin.clone()))
        ref = _closed_form(c, idx, nz, pairs, beta, p_global)
        o32, o64 = _oracle(c, idx, nz, torch.float32, pairs, beta, p_global), _oracle(c, idx, nz, torch.float64, pairs, beta, p_global)
        assert torch.count_nonzero(o32["preds"][0]) == 0 and torch.count_nonzero(o32["preds"][1]) == 0 and float(ref["m"].abs().min()) > 0
        checks += [((delta, ref["delta"], o32["delta"], f"{what} step {k} d_b"), {}), ((margin, ref["m"], o32["m"], f"{what} step {k} m_p"), {})]
        new = dict(st=ref["stats"], st32=o32["stats"].double(), bias=ref["bias"], **{n: o64["grads"][n] for n in NAMES[:3]},
                   **{n + "32": o32["grads"][n].double() for n in NAMES})
        tot = new if tot is None else {n: tot[n] + v for n, v in new.items()}
    dev = TA._grads(c.m, grad)
    checks += [((stats[r:r + 1], tot["st"][r:r + 1], tot["st32"][r:r + 1], f"{what} statistics row {r}"), {}) for r in range(3)]
    checks += [((dev["type_out.bias"], tot["bias"], tot[NAMES[3] + "32"], f"{what} grad type_out.bias vs sum of seeds"), {})]
    checks += [((dev[n[len("decoder."):]], tot[n], tot[n + "32"], f"{what} grad {n}"), {}) for n in NAMES[:3]]
    FA._all(checks)
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(stats).all())
    TA._assert_trunk_gradient_is_zero(c.m, grad)
    return grad, stats, outs


# ---- 1. zero heads, loop shapes -------------------------------------------------------------------------------------------------------

def test_zero_heads_at_the_loop_shapes_vs_float64():
    """Two mi_dpo_micro_step calls (t = 433 and t = 1) into one gradient and one statistics buffer, injected noise, p_global = 7 > P = 5,
    accum_steps = 3: out_delta, out_margin, the three statistics rows, the type_out.bias gradient and the head weights' gradients against
    the reference; every trunk gradient exactly zero.  Crystal 4 sits in no pair, so its coefficient is 0 and nothing of it may reach the
    result: the same two calls on a set whose crystal 4 carries OTHER noise (other targets: any non-zero coefficient would move the type_out.bias
    gradient) give, by torch.equal, the same statistics, margins, d_b of the paired crystals and type_out.bias gradient."""
    c = FA._case("loop")
    idxs, p_global = (T - 433, T - 1), 7
    grad, stats, outs = _zero_head_steps(c, idxs, LOOP_PAIRS, BETA, p_global, "loop")
    n2g = R._batch(c.na)[1]
    grad2, stats2 = torch.zeros_like(grad), torch.zeros_like(stats)
    others = torch.tensor([b for b in range(c.B) if b != 4], device="cuda")
    for k, idx in enumerate(idxs):
        zl, zx, zt = (v.clone() for v in R.noise(c.fs, seed=40 + k))
        g = torch.Generator().manual_seed(900 + k)
        zl[4], zt[n2g == 4] = torch.randn(3, 3, generator=g), torch.randn(int((n2g == 4).sum()), R.NUM_TYPES, generator=g)
        delta, margin = _dpo_micro(c, idx, (zl, zx, zt), LOOP_PAIRS, BETA, grad2, stats2, p_global)
        assert torch.equal(margin, outs[k][1]) and torch.equal(delta[others], outs[k][0][others]) and not torch.equal(delta[4], outs[k][0][4])
    assert torch.equal(stats2, stats)
    assert torch.equal(TA._grads(c.m, grad2)["type_out.bias"], TA._grads(c.m, grad)["type_out.bias"])
    TA._assert_trunk_gradient_is_zero(c.m, grad2)


# ---- 2. many crystals, many pairs -----------------------------------------------------------------------------------------------------

def test_zero_heads_at_300_crystals_and_600_pairs_vs_float64():
    """GRID_NA with 600 pairs, 300 of them won by crystal 0: a second trip of the per-crystal slot loop and of the pair loop, the
    statistics sums over 600 terms, a second (partial) block of the time fill."""
    _zero_head_steps(FA._case("grid"), (T - 433,), GRID_PAIRS, BETA, len(GRID_PAIRS), "grid")


# ---- 3. saturation --------------------------------------------------------------------------------------------------------------------

def test_saturated_pairs_stay_finite_and_match_the_reference():
    """The loop set with beta chosen so that max|u_p| >= 200 with both signs present (asserted on the reference): everything finite, the
    loss row (= sum_p softplus(u_p) / p_global ~ sum_p max(u_p, 0) / p_global) and the gradients against the reference."""
    c = FA._case("loop")
    ref = _closed_form(c, T - 433, R.noise(c.fs, seed=40), LOOP_PAIRS, 1.0, 7)
    beta = 400.0 / float(ref["m"].abs().max())
    u = _closed_form(c, T - 433, R.noise(c.fs, seed=40), LOOP_PAIRS, beta, 7)["u"]
    assert float(u.abs().max()) >= 200 and float(u.min()) < 0 < float(u.max())
    grad, stats, _ = _zero_head_steps(c, (T - 433,), LOOP_PAIRS, beta, 7, "saturated")
    # (softplus(u) - max(u, 0) = log1p(exp(-|u|)) <= log 2 per pair)
    assert 0 <= float(stats[0]) - float(u.clamp(min=0).sum()) / 7 + 1e-4 * float(u.abs().max()) <= len(LOOP_PAIRS) * np.log(2) / 7 + 2e-4 * float(u.abs().max())


# ---- 4. near-equal networks -----------------------------------------------------------------------------------------------------------

def test_delta_at_nearly_equal_networks_needs_the_factorised_form():
    """Zero heads, prior bias = agent bias + 1e-4 randn: out_delta within the rule's tolerance relative to max|d_b|, the yardstick being
    the FACTORISED float32 formula on the CPU.  The direct difference of the two reduced losses in float32 misses that tolerance (asserted
    here, so the case cannot go soft): a kernel that forms d_b that way fails."""
    P = TA._params(1, seed=3)[1]
    Q = {k: v.clone() for k, v in P.items()}
    Q["decoder.type_out.bias"] = P["decoder.type_out.bias"] + 1e-4 * torch.randn(100, generator=torch.Generator().manual_seed(77))
    c = FA._make(FA.LOOP_NA, P, Q, seed=21)
    FA._offsets(c)
    idx, nz = T - 433, R.noise(c.fs, seed=44)
    grad, stats = torch.zeros_like(c.m.decoder.theta), torch.zeros(3, device="cuda")
    delta, margin = _dpo_micro(c, idx, nz, LOOP_PAIRS, BETA, grad, stats, 7)
    out = R.add_noise(c.fs, R.schedule(c.tables, [T - idx] * c.B), nz)
    pa, pp, tg = R.zero_head_preds(c.na, c.bias_a), R.zero_head_preds(c.na, c.bias_p), (out["rand_l"], out["tar_x"], out["rand_t"])
    tg32 = R.oracle_add_noise(c.tables, c.fs, nz, torch.float32, idx)[1]
    ref = D.delta(pa, pp, tg, R.COSTS, c.na)
    fac32, dir32 = D.delta(pa, pp, tg32, R.COSTS, c.na, torch.float32), D.delta_direct(pa, pp, tg32, R.COSTS, c.na, torch.float32)
    scale = float(ref.abs().max())
    tol = max(4 * float((fac32.double() - ref).abs().max()) / scale, FA.FLOOR)
    assert scale < 1e-2 and float((dir32.double() - ref).abs().max()) / scale > 10 * tol, "the direct float32 form must miss the tolerance"
    FA._check(delta, ref, fac32, "near-equal networks d_b")
    FA._check(margin, D.pair_terms(ref, LOOP_PAIRS, BETA)[0], D.pair_terms(fac32, LOOP_PAIRS, BETA)[0], "near-equal networks m_p")
    assert bool(torch.isfinite(grad).all())


# ---- 5. non-zero heads ----------------------------------------------------------------------------------------------------------------

def test_micro_step_with_nonzero_heads_at_86_atoms_vs_float64_oracle():
    """Agent != prior, head_scale = 0.1, na = [86, 3, 1], one micro-step at t = HEADS_T: out_delta, out_margin, the statistics and every
    gradient tensor against the oracle (add_noise + both forwards + the preference loss + autograd) in float64 on the CPU.  Tolerance: the
    yardstick's, never looser than tests/test_gpu_train.py's test_ft_gradients_and_adam_golden (2e-5 per gradient tensor).

    The time: the crystals' coefficients c_b sum to zero, so a parameter's gradient is a DIFFERENCE of per-crystal gradients, and what all
    of them share is amplified relative to it -- here the float32 time embedding sin / cos(t f), whose argument carries a rounding error
    proportional to t.  At t = 433 the float32 formulas on the CPU are themselves 2.3e-5 of max|ref| off float64 (final_layer_norm.weight;
    2.1e-5 node_embedding.bias, 1.9e-5 atom_latent_emb.weight): above the cap, which would then ask for more than float32 gives.  At
    t = 100 they are 3.2e-6 at worst, four times that is under the cap (asserted below), and the cap binds nothing the rule does not."""
    c = FA._make(FA.HEADS_NA, TA._params(1, seed=7, zero_heads=False)[1], TA._params(1, seed=8, zero_heads=False)[1], seed=23)
    FA._offsets(c)
    nz = R.noise(c.fs, seed=60)
    grad, stats = torch.zeros_like(c.m.decoder.theta), torch.zeros(3, device="cuda")
    delta, margin = _dpo_micro(c, T - HEADS_T, nz, HEADS_PAIRS, BETA, grad, stats, 4)
    o64, o32 = _oracle(c, T - HEADS_T, nz, torch.float64, HEADS_PAIRS, BETA, 4), _oracle(c, T - HEADS_T, nz, torch.float32, HEADS_PAIRS, BETA, 4)
    assert float(o64["preds"][0].abs().max()) > 1e-3 and float(o64["preds"][1].abs().max()) > 1e-3 and float(o64["m"].abs().min()) > 0
    checks = [((delta, o64["delta"], o32["delta"], "non-zero heads d_b"), dict(cap=2e-4)), ((margin, o64["m"], o32["m"], "non-zero heads m_p"), dict(cap=2e-4))]
    checks += [((stats[r:r + 1], o64["stats"][r:r + 1], o32["stats"][r:r + 1], f"non-zero heads statistics row {r}"), dict(cap=2e-4)) for r in range(3)]
    for k, g in TA._grads(c.m, grad).items():
        r64, r32 = o64["grads"]["decoder." + k], o32["grads"]["decoder." + k].double()
        assert float(r64.abs().max()) > 0 and 4 * float((r32 - r64).abs().max()) <= 2e-5 * float(r64.abs().max()), k
        checks.append(((g, o64["grads"]["decoder." + k], o32["grads"]["decoder." + k], f"non-zero heads grad {k}"), dict(cap=2e-5)))
    FA._all(checks)


# ---- 6. device noise ------------------------------------------------------------------------------------------------------------------

def test_device_noise_vs_the_host_philox_contract():
    """One micro-step with the device's own draws on a shard that starts at atom NODE_OFF, crystal GRAPH_OFF: out_delta and out_margin
    against the reference fed the host contract's draws 7-9 at the call id, with the first-order bound of the draws' libm round-off added;
    a second call with the same call id gives the same bits."""
    c = FA._case("loop")
    FA._offsets(c, FA.NODE_OFF, FA.GRAPH_OFF)
    call, idx = 41, T - 433
    try:
        grad, stats = torch.zeros_like(c.m.decoder.theta), torch.zeros(3, device="cuda")
        delta, margin = _dpo_micro(c, idx, None, LOOP_PAIRS, BETA, grad, stats, 7, call_id=call)
        grad2, stats2 = torch.zeros_like(grad), torch.zeros_like(stats)
        delta2, margin2 = _dpo_micro(c, idx, None, LOOP_PAIRS, BETA, grad2, stats2, 7, call_id=call)
    finally:
        FA._offsets(c)
    assert torch.equal(delta, delta2) and torch.equal(margin, margin2) and torch.equal(grad, grad2) and torch.equal(stats, stats2)
    nz = FA._philox(call, c.B, c.N)
    zs = tuple(v.double().requires_grad_(True) for v in nz)
    ref = _closed_form(c, idx, zs, LOOP_PAIRS, BETA, 7)
    o32 = _oracle(c, idx, nz, torch.float32, LOOP_PAIRS, BETA, 7)
    FA._all([((delta, ref["delta"], o32["delta"], "device noise d_b"), dict(slack=FA._first_order(ref["delta"], zs))),
             ((margin, ref["m"], o32["m"], "device noise m_p"), dict(slack=FA._first_order(ref["m"], zs)))])
    TA._assert_trunk_gradient_is_zero(c.m, grad)


# ---- 7. no leak into the fine-tune entry ----------------------------------------------------------------------------------------------

def test_pairs_and_a_dpo_step_leave_the_fine_tune_entry_its_bits():
    """mi_ft_micro_step's gradient and statistics on the same handles before mi_batch_set_pairs, after it, and after a mi_dpo_micro_step:
    all three torch.equal."""
    c = FA._case("loop")
    FA._offsets(c)
    idx, nz, b_global = T - 433, R.noise(c.fs, seed=40), 2 * c.B

    def ft():
        grad, stats = torch.zeros_like(c.m.decoder.theta), torch.zeros(3, device="cuda")
        Lb, KLb = FA._micro(c, idx, nz, grad, stats, b_global)
        return grad, stats, Lb, KLb
    torch.cuda.synchronize()
    _handle(c).set_pairs(None)
    assert _handle(c).num_pairs == 0
    before = ft()
    _handle(c).set_pairs(LOOP_PAIRS)
    assert _handle(c).num_pairs == len(LOOP_PAIRS)
    with_pairs = ft()
    _dpo_micro(c, idx, nz, LOOP_PAIRS, BETA, torch.zeros_like(c.m.decoder.theta), torch.zeros(3, device="cuda"), 7)
    after = ft()
    for other in (with_pairs, after):
        assert all(torch.equal(a, b) for a, b in zip(before, other))
    assert float(before[0].abs().max()) > 0


# ---- 8. dpo_step end to end -----------------------------------------------------------------------------------------------------------

E2E_NA, E2E_PAIRS, E2E_BETA, E2E_SEED = [4, 2, 6, 3], [(0, 1), (2, 1), (0, 3)], 1.0, 9


@functools.lru_cache(maxsize=None)
def _e2e_inputs(seed=E2E_SEED):
    """The configuration of tests/test_gpu_train.py's test_ft_step_end_to_end_vs_oracle (H = 64, L = 2, F = 8, agent = prior + 0.01 randn,
    injected noise for 2 epochs x 6 timesteps) and the oracle's run of the whole step on it (float32, CPU): built once."""
    from matinvent_amd.data import CrystalData
    hp = O.CSPNetHParams(hidden_dim=64, num_layers=2, num_freqs=8)
    P0, Q0 = O.init_params(hp, seed=3), O.init_params(hp, seed=3)
    gen = torch.Generator().manual_seed(seed)
    for k in P0:
        P0[k] = P0[k] + 0.01 * torch.randn(P0[k].shape, generator=gen)
    sn = torch.cat([torch.ones(1), 0.5 + torch.rand(1000, generator=gen)])
    na = E2E_NA
    data = [CrystalData(torch.rand(n, 3, generator=gen), torch.randint(1, 95, (n,), generator=gen), 4 + 6 * torch.rand(1, 3, generator=gen),
                        70 + 40 * torch.rand(1, 3, generator=gen)) for n in na]
    B, N = len(na), sum(na)
    noises = {(e, t): (torch.randn(B, 3, 3, generator=gen), torch.randn(N, 3, generator=gen), torch.randn(N, 100, generator=gen))
              for e in range(2) for t in range(6)}
    sch = O.Schedules.make(1000, sigmas_norm=sn)
    batch = dict(num_atoms=torch.tensor(na), lengths=torch.cat([d.lengths for d in data]), angles=torch.cat([d.angles for d in data]),
                 frac_coords=torch.cat([d.frac_coords for d in data]), atom_types=torch.cat([d.atom_types for d in data]))
    return dict(hp=hp, P0=P0, Q0=Q0, sn=sn, data=data, noises=noises, sch=sch, batch=batch)


def _e2e_oracle(x, beta_sched=None):
    sch = x["sch"]
    if beta_sched is not None:
        sch.beta = beta_sched
    A, rec = {k: v.clone() for k, v in x["P0"].items()}, {}
    D.oracle_dpo_step(A, x["Q0"], x["hp"], sch, O.Costs(), x["batch"], E2E_PAIRS,
                      lambda e, t: dict(zip(("rand_l", "rand_x", "rand_t"), x["noises"][(e, t)])), lr=1e-4, timesteps=6, accum_steps=3,
                      beta=E2E_BETA, epochs=2, record=rec)
    return A, rec


def test_dpo_step_end_to_end_vs_oracle():
    """preference.dpo_step vs dpo_ref64.oracle_dpo_step: 2 epochs x 6 timesteps, accum 3 -> 4 optimizer steps, lr 1e-4, injected noise,
    pairs [(0, 1), (2, 1), (0, 3)].  test_ft_step_end_to_end_vs_oracle's acceptance: every parameter within 1.2e-4, 98 % within 1e-5, the
    logged loss within 1e-4 max(1, |ref|).  pref_acc is exact as a count: no |m_p| of the reference's run lies near 0 (asserted)."""
    from matinvent_amd.preference import dpo_step
    x = _e2e_inputs()
    agent, prior = make_module(64, 2, 8, 1000, x["P0"], sigmas_norm=x["sn"]), make_module(64, 2, 8, 1000, x["Q0"], sigmas_norm=x["sn"])
    prior.requires_grad_(False)
    calls0 = getattr(agent, "_noise_calls", 0)
    cfg = dict(lr=1e-4, accum_steps=3, epochs=2, timesteps=6, dpo_beta=E2E_BETA)
    stats = dpo_step(agent, prior, x["data"], E2E_PAIRS, cfg, noise_fn=lambda e, t: x["noises"][(e, t)])
    assert agent._noise_calls == calls0 + 12 and len(stats) == 2 and list(stats[0]) == ["loss", "pref_acc", "margin"]
    assert agent._batch_for(torch.tensor(E2E_NA)).num_pairs == 0                  # (the cached handle is left without pairs)
    A, rec = _e2e_oracle(x, {k: getattr(agent.beta_scheduler, k).cpu() for k in ("betas", "alphas", "alphas_cumprod", "sigmas")})
    m = torch.stack(rec["m"])
    assert float(m.abs().min()) > 1e-3 * float(m.abs().max()), "choose another E2E_SEED: a margin of the reference lies near 0"
    for k, w in agent.decoder.views().items():
        d = (w.detach().cpu() - A["decoder." + k]).abs()
        assert float(d.max()) <= 1.2e-4, f"{k}: {float(d.max())}"
        assert float(d.flatten().kthvalue(max(1, int(0.98 * d.numel()))).values) <= 1e-5, k
    assert float((agent.decoder.theta.detach().cpu() - make_module(64, 2, 8, 1000, x["P0"], sigmas_norm=x["sn"]).decoder.theta.detach().cpu()).abs().max()) > 0
    for e in range(2):
        ref_loss = float(torch.stack(rec["loss"][6 * e:6 * e + 6]).sum() / 6)
        assert abs(stats[e]["loss"] - ref_loss) <= 1e-4 * max(1.0, abs(ref_loss))
        assert stats[e]["pref_acc"] == pytest.approx(float((m[6 * e:6 * e + 6] < 0).sum()) / 6 / len(E2E_PAIRS), abs=1e-6)
        ref_margin = float(-m[6 * e:6 * e + 6].sum() / 6 / len(E2E_PAIRS))
        assert abs(stats[e]["margin"] - ref_margin) <= 1e-4 * max(1.0, abs(ref_margin))


# ---- 9. validation --------------------------------------------------------------------------------------------------------------------

def test_set_pairs_validation_and_the_micro_step_without_pairs():
    """An out-of-range index, w == l and n_pairs < 0 each give MI_EINVAL and leave num_pairs as it was; mi_dpo_micro_step on a handle
    without pairs gives MI_ESTATE and touches neither the gradient nor the statistics."""
    import ctypes as C
    from matinvent_amd import _lib, preference
    c = FA._case("loop")
    FA._offsets(c)
    torch.cuda.synchronize()
    ab = _handle(c)
    ab.set_pairs(LOOP_PAIRS)
    for bad in ([(0, c.B)], [(-1, 2)], [(3, 3)], [(0, 1), (2, 2)]):
        with pytest.raises(_lib.MIError) as e:
            ab.set_pairs(bad)
        assert e.value.code == _lib.MI_EINVAL and ab.num_pairs == len(LOOP_PAIRS)
    arr = (C.c_int * 1)(0)
    assert _lib.load().mi_batch_set_pairs(ab._h, arr, arr, -1) == _lib.MI_EINVAL and ab.num_pairs == len(LOOP_PAIRS)
    assert _lib.load().mi_batch_set_pairs(ab._h, None, arr, 1) == _lib.MI_EINVAL and ab.num_pairs == len(LOOP_PAIRS)
    ab.set_pairs(None)
    assert ab.num_pairs == 0
    grad, stats = torch.full_like(c.m.decoder.theta, 3.0), torch.full((3,), 7.0, device="cuda")
    with pytest.raises(_lib.MIError) as e:
        preference._dpo_micro_step(c.m, c.prior, c.batch, T - 433, R.noise(c.fs, seed=40), BETA, 7, ACCUM, grad, stats, call_id=1)
    torch.cuda.synchronize()
    assert e.value.code == _lib.MI_ESTATE and bool((grad == 3.0).all()) and bool((stats == 7.0).all())


# ---- 10. the pipeline -----------------------------------------------------------------------------------------------------------------

def test_dropin_main_runs_the_dpo_pipeline_with_what_the_policy_gradient_refuses(tmp_path):
    """dropin/main.py pipeline=mat_invent_dpo, two loops, with replay, the diversity filter, a fixed formula (conditioned sampling) and a
    strided chain -- the combination MatInventPG refuses: it runs, logs dpo_loss / pref_acc / margin / pairs, pairs >= 1, and the agent's
    parameters moved and are finite."""
    import csv
    import tests.test_gpu_respaced_chain as RC
    from matinvent_amd.pipeline import MatInventDPO
    tiny = [a for a in RC.TINY if not a.startswith("rl_epoch=")] + ["rl_epoch=2"]
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        import main as dropin_main
        np.random.seed(0)
        rl = dropin_main.main(["expname=dpo", "pipeline=mat_invent_dpo", "pipeline.finetune_cfg.timesteps=6", "pipeline.finetune_cfg.accum_steps=3",
                               "pipeline.finetune_cfg.epochs=1", "pipeline.finetune_cfg.dpo_beta=1.0", "pipeline.replay=True", "reward.mode=uniform",
                               "pipeline.replay_args.reward_cutoff=0.0", "pipeline.div_filter=true", "+pipeline.df_args={tol: 5, buff: 12}",
                               "+sample_cfg.target_compositions_dict=[{Li: 2, O: 1}]"] + tiny)
    finally:
        os.chdir(cwd)
        sys.path.remove(os.path.join(ROOT, "dropin"))
    assert isinstance(rl, MatInventDPO) and rl.replay is not None and rl.div_filter and rl.sample_steps == 5
    assert [dict(d) for d in rl.sample_cfg.target_compositions_dict] == [{"Li": 2, "O": 1}]
    rows = list(csv.DictReader(open(tmp_path / "exp_res" / "dpo" / "metrics.csv")))
    assert len(rows) == 2
    for r in rows:
        for k in ("dpo_loss", "pref_acc", "margin", "pairs"):
            assert k in r and np.isfinite(float(r[k])), (k, r)
        assert float(r["pairs"]) >= 1 and 0.0 <= float(r["pref_acc"]) <= 1.0
    assert len(rl.replay) > 0
    theta = rl.agent.decoder.theta.detach()
    assert bool(torch.isfinite(theta).all())
    assert 0 < float((theta - rl.prior.decoder.theta).abs().max()) < 1e-2

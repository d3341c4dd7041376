"""GPU checks of the fine-tune micro-step's own kernels (matinvent_amd/csrc/backward.hip: add_noise_kernel, ft_loss_kernel,
ft_stats_kernel, fill_stack_times_kernel under ft_micro_impl) against the float64 reference tests/ft_ref64.py, with the network taken
out of the comparison and at the sizes the kernels loop over.

With the three head weight matrices of the agent AND of the prior zero, both networks predict exactly pl = 0, px = 0, pt = their own
type_out.bias, whatever the trunks compute: L_b, KL_b (one constant per crystal, not 0: the biases differ), the three statistics rows and
the type_out.bias gradient sum_i seed_t[i, :] are closed forms of the set, the noise and the two biases; the gradient of every trunk
tensor is exactly zero, that of the head weights seeds^T h.

Network and schedule: H = 64, L = 1, F = 8; the T = 1000 cosine schedule, sigmas_norm as tests/test_gpu_traj_arithmetic._module.
Atom counts: LOOP_NA = [1, 2, 85, 86, 3, 171] -- 3n = 255, 258, 513: one, two and three trips of the 256-thread coordinate loops of
add_noise_kernel and ft_loss_kernel, the last one partial, and up to 67 trips of their type loops; no count is a multiple of 4.
GRID_NA = 300 crystals of 1..3 atoms: ft_stats_kernel's serial loop, and a second, partial block of the per-crystal time fill and of
the time embedding (seen through the head weights' gradients, seeds^T h).  STACK_NA = [2, 86, 3] in 3 replicas: the stacked entry.
The sets (ft_ref64.build_set) hold the edge values: coordinates exactly 0 and nextafter(1, 0) whose noise crosses the cell boundary
(the last coordinate of every crystal, so in the last partial trip), atom types 1 and 100, angles 90/90/90 and 60/60/60, rewards
exactly 0, 1 and 1.1; the times include t = 1 (sigma = sigma_begin: every image but one underflows in d_log_p_wn) and t = T.

Tolerances (measured in the test, not guessed; DESIGN 25's rule): the yardstick of a quantity is the deviation of the float32 formulas
run on the CPU (oracle.diffcsp_oracle in float32 through ft_ref64.oracle_micro_step / oracle_add_noise: the same separately rounded
tensor ops as DiffCSPModule.calc_sample_loss / calc_kl_reg and finetune's accumulation, same inputs) from float64, relative to
max|ref64|; the device gets 4 times that, at least 4 * 2^-24.  in_frac is compared on the circle (min(|d|, 1 - |d|), scale 1: the cell).
Where the device draws its own noise the reference is fed the host Philox contract's draws, which the device's differ from by Box-Muller
libm round-off (the project's atol 5e-6, tests/test_gpu_forward.test_philox_matches_contract): a quantity then also gets 5e-6 times
the sum of the reference's absolute first derivatives with respect to the draws (float64 autograd) -- the first-order bound of what
that round-off can move, nothing more.  MI_TOL_REPORT=1 prints yardstick, device error and tolerance."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tests.test_gpu_traj_arithmetic as TA
from oracle import diffcsp_oracle as O
from tests import ft_ref64 as R

pytestmark = pytest.mark.gpu

T = 1000
FLOOR = 4 * 2.0 ** -24
LOOP_NA = [1, 2, 85, 86, 3, 171]
GRID_NA = [1, 3, 2] * 100
STACK_NA = [2, 86, 3]
HEADS_NA = [86, 3, 1]
SIGMA_KL, ACCUM = 0.025, 3
SEED = 1234
NODE_OFF, GRAPH_OFF = 1000003, 4099        # 3 * NODE_OFF = 1 and 9 * GRAPH_OFF = 3 (mod 4): the draws start inside a Philox quad
PHILOX_ATOL = 5e-6
IDX = {"t=1": T - 1, "t=T": 0, "t=433": T - 433}
HEADS = TA.HEADS


def test_the_shapes_reach_what_they_are_chosen_for():
    """Arithmetic facts of the shapes (no device work): a later edit of the shapes must not silently lose them."""
    assert [3 * n for n in LOOP_NA if 3 * n > 200] == [255, 258, 513]
    assert all(n % 4 for n in LOOP_NA + STACK_NA + HEADS_NA)
    assert 256 < len(GRID_NA) < 512 and sum(GRID_NA) <= 600 and max(LOOP_NA) == 171
    assert (3 * NODE_OFF) % 4 and (9 * GRAPH_OFF) % 4 and 3 * max(STACK_NA) > 256 and 3 * max(HEADS_NA) > 256


# ---- helpers ------------------------------------------------------------------------------------------------------------------------

def _check(dev, ref64, ref32, what, circle=False, slack=0.0, cap=None):
    """dev within max(4 x the fp32 formulas' own deviation from float64, 4 * 2^-24) of max|ref64| (never more than `cap`), plus `slack`
    (absolute: what the Philox draws' libm round-off can move).  circle: distances on the unit circle, scale 1."""
    dev, ref64, ref32 = (v.detach().double().cpu() for v in (dev, ref64, ref32))
    assert dev.shape == ref64.shape == ref32.shape, (what, dev.shape, ref64.shape, ref32.shape)
    dist = (lambda a, b: torch.minimum((a - b).abs(), 1 - (a - b).abs())) if circle else (lambda a, b: (a - b).abs())
    scale = 1.0 if circle else max(1e-300, float(ref64.abs().max()))
    yard = float(dist(ref32, ref64).max()) / scale
    err = float(dist(dev, ref64).max()) / scale
    tol = max(4 * yard, FLOOR)
    if cap is not None:
        tol = min(tol, cap)
    tol += float(slack) / scale
    if os.environ.get("MI_TOL_REPORT"):
        print(f"TOL {what}: fp32 reference {yard:.3e}, device {err:.3e} of max|ref| = {scale:.3g}, demanded {tol:.3e}"
              + (f" (of it Philox round-off {float(slack) / scale:.3e})" if slack else ""))
    assert bool(torch.isfinite(dev).all()) and err <= tol, f"{what}: device error {err:.3e} of max|ref| ({scale:.3g}) > {tol:.3e} (fp32 reference: {yard:.3e})"


def _all(checks):
    """Run every (args, kwargs) of `checks` through _check and report all the failures together."""
    bad = []
    for args, kw in checks:
        try:
            _check(*args, **kw)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)


def _tables(m):
    return dict(alphas_cumprod=m.beta_scheduler.alphas_cumprod.cpu(), sigmas=m.sigma_scheduler.sigmas.cpu(),
                sigmas_norm=m.sigma_scheduler.sigmas_norm.cpu())


def _make(na, P, Q, seed):
    c = SimpleNamespace(hp=O.CSPNetHParams(hidden_dim=TA.H, num_layers=1, num_freqs=TA.F), P=P, Q=Q, na=na, B=len(na), N=sum(na),
                        m=TA._module(1, P), prior=TA._module(1, Q))
    c.prior.requires_grad_(False)
    c.m.noise_seed = SEED
    c.fs = R.build_set(na, seed=seed)
    c.batch = SimpleNamespace(**{k: c.fs[k] for k in R.SET_KEYS + ("reward",)})
    c.tables, c.freqs = _tables(c.m), c.m.time_embedding.freqs.cpu()
    c.bias_a, c.bias_p = P["decoder.type_out.bias"], Q["decoder.type_out.bias"]
    return c


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Zero heads on both networks (different biases, different trunks), one set per shape: built once, shared, left unchanged."""
    na = {"loop": LOOP_NA, "grid": GRID_NA, "stack": STACK_NA}[shape]
    return _make(na, TA._params(1, seed=3)[1], TA._params(1, seed=4)[1], seed=21)


def _offsets(c, node=0, graph=0):
    c.m.shard_offsets = c.prior.shard_offsets = (node, graph)


def _philox(call, B, N):
    """The host contract's draws of one fine-tune noise call for a shard starting at atom NODE_OFF, crystal GRAPH_OFF."""
    f = lambda draw, n, off, *shape: torch.from_numpy(O.philox_normal(SEED, call, draw, n, off).copy()).view(*shape)
    return (f(O.DRAW_FT_L, B * 9, GRAPH_OFF * 9, B, 3, 3), f(O.DRAW_FT_X, N * 3, NODE_OFF * 3, N, 3),
            f(O.DRAW_FT_T, N * R.NUM_TYPES, NODE_OFF * R.NUM_TYPES, N, R.NUM_TYPES))


def _first_order(outputs, zs):
    """PHILOX_ATOL x sum |d output / d z| per element of `outputs` (float64 autograd graph on the leaves `zs`), the largest one."""
    worst = 0.0
    for o in outputs.reshape(-1):
        g = torch.autograd.grad(o, zs, retain_graph=True, allow_unused=True)
        worst = max(worst, PHILOX_ATOL * sum(float(v.abs().sum()) for v in g if v is not None))
    return worst


def _closed_form(c, idx, nz, b_global):
    """One zero-head micro-step at time index idx in float64: (L_b, KL_b, the three statistics rows, the type_out.bias gradient)."""
    out = R.add_noise(c.fs, R.schedule(c.tables, [T - idx] * c.B), nz)
    pa, pp, tg = R.zero_head_preds(c.na, c.bias_a), R.zero_head_preds(c.na, c.bias_p), (out["rand_l"], out["tar_x"], out["rand_t"])
    L, KL = R.loss_kl(pa, pp, tg, R.COSTS, c.na)
    sd = R.seeds(pa, pp, tg, R.COSTS, c.na, c.fs["reward"], SIGMA_KL, b_global, ACCUM)
    return L, KL, R.stats(L, KL, c.fs["reward"], SIGMA_KL, b_global), sd[2].sum(dim=0)


def _oracle(c, idx, nz, dtype, b_global):
    return R.oracle_micro_step(c.hp, c.P, c.Q, c.tables, c.fs, nz, dtype, time_idx=idx, sigma=SIGMA_KL, b_global=b_global, accum=ACCUM,
                               freqs=c.freqs, grad=True)


def _micro(c, idx, nz, grad, stats, b_global, call_id=1):
    """mi_ft_micro_step called directly, with real out_sample_loss / out_kl buffers; returns them."""
    from matinvent_amd import _lib, finetune
    from matinvent_amd.cspnet import _ptr, _stream
    head, (t,), sched, dz, aux = finetune._micro_step_operands(c.m, c.prior, c.batch, [idx], None if nz is None else [nz], None)
    Lb, KLb = torch.full((c.B,), float("nan"), device="cuda"), torch.full((c.B,), float("nan"), device="cuda")
    _lib.check(_lib.load().mi_ft_micro_step(*head, t, *(s[0] for s in sched), SEED, call_id, _ptr(dz[0]), _ptr(dz[1]), _ptr(dz[2]),
                                            *R.COSTS, SIGMA_KL, b_global, ACCUM, _ptr(grad), _ptr(stats), _ptr(Lb), _ptr(KLb), _stream(), aux),
               "mi_ft_micro_step")
    torch.cuda.synchronize()
    return Lb, KLb


# ---- (a) add_noise alone ------------------------------------------------------------------------------------------------------------

def _noise_checks(dev, ref, r32, what, slack=None):
    """Every output of add_noise: dev = DiffCSPModule.add_noise's triple, ref = ft_ref64.add_noise's dict, r32 = the float32 oracle's triple."""
    (_, in_types, in_frac, in_lat, _, _), (rand_l, tar_x, rand_t), _ = dev
    (_, t32, f32, l32, _, _), (rl32, tx32, rt32), _ = r32
    slack = slack or {}
    return [((d, ref[k], o, f"{what} {k}"), dict(circle=k == "in_frac", slack=slack.get(k, 0.0)))
            for k, d, o in (("in_lat", in_lat, l32), ("in_types", in_types, t32), ("in_frac", in_frac, f32), ("tar_x", tar_x, tx32),
                            ("rand_l", rand_l, rl32), ("rand_t", rand_t, rt32))]


def _sampled_times(B, seed):
    """Per-crystal times as add_noise(time=None) draws them (numpy's global generator); the generator is left seeded for that call."""
    np.random.seed(seed)
    times = np.random.choice(np.arange(1, T + 1), B).tolist()
    np.random.seed(seed)
    return times


@pytest.mark.parametrize("when", ["t=1", "t=T", "t=433", "per-crystal"])
def test_add_noise_with_injected_noise_vs_float64(when):
    """DiffCSPModule.add_noise(batch, time, noise=...) at LOOP_NA: all six outputs at t = 1, t = T, in between and with one time per crystal."""
    c = _case("loop")
    _offsets(c)
    nz = R.noise(c.fs, seed=31)
    times, kw = ([T - IDX[when]] * c.B, dict(time_idx=IDX[when])) if when in IDX else (_sampled_times(c.B, 5), {})
    if not kw:
        kw = dict(times=times)
    with torch.no_grad():
        dev = c.m.add_noise(c.batch, IDX.get(when), noise=nz)
    ref = R.add_noise(c.fs, R.schedule(c.tables, times), nz)
    _all(_noise_checks(dev, ref, R.oracle_add_noise(c.tables, c.fs, nz, torch.float32, **kw), f"add_noise {when}"))
    assert torch.equal(dev[1][0].cpu(), nz[0]) and torch.equal(dev[1][2].cpu(), nz[2])       # (the targets are the injected draws themselves)
    assert float(dev[0][2].min()) >= 0 and float(dev[0][2].max()) <= 1


@pytest.mark.parametrize("when", ["t=1", "t=433", "per-crystal"])
def test_add_noise_with_device_noise_vs_the_host_philox_contract(when):
    """noise=None on a batch handle of a shard that starts at atom NODE_OFF, crystal GRAPH_OFF: the returned rand_l / rand_t are the host
    contract's draws 7 / 9 at the call id, the global element ids and the shard offsets (atol 5e-6); in_frac and tar_x follow from draw 8."""
    c = _case("loop")
    _offsets(c, NODE_OFF, GRAPH_OFF)
    call = 41
    c.m._noise_calls = call - 1
    times, kw = ([T - IDX[when]] * c.B, dict(time_idx=IDX[when])) if when in IDX else (_sampled_times(c.B, 6), {})
    if not kw:
        kw = dict(times=times)
    try:
        with torch.no_grad():
            dev = c.m.add_noise(c.batch, IDX.get(when))
    finally:
        _offsets(c)
    assert c.m._noise_calls == call
    nz = _philox(call, c.B, c.N)
    np.testing.assert_allclose(dev[1][0].cpu().numpy(), nz[0].numpy(), rtol=0, atol=PHILOX_ATOL)
    np.testing.assert_allclose(dev[1][2].cpu().numpy(), nz[2].numpy(), rtol=0, atol=PHILOX_ATOL)
    sched = R.schedule(c.tables, times)
    zx = nz[1].double().requires_grad_(True)
    ref = R.add_noise(c.fs, sched, (nz[0], zx, nz[2]))
    dtx, = torch.autograd.grad(ref["tar_x"].sum(), zx)          # (element-wise map: the gradient of the sum is each element's derivative)
    slack = dict(in_lat=PHILOX_ATOL * float(sched[:, 1].max()), in_types=PHILOX_ATOL * float(sched[:, 1].max()),
                 in_frac=PHILOX_ATOL * float(sched[:, 2].max()), tar_x=PHILOX_ATOL * float(dtx.abs().max()), rand_l=PHILOX_ATOL, rand_t=PHILOX_ATOL)
    _all(_noise_checks(dev, ref, R.oracle_add_noise(c.tables, c.fs, nz, torch.float32, **kw), f"add_noise, device noise, {when}", slack))


# ---- (b) the fused micro-step, zero heads ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,idxs", [("loop", (T - 1, T - 433)), ("grid", (0, T - 433))], ids=["loop", "grid"])
def test_fused_micro_steps_with_zero_heads_vs_float64(shape, idxs):
    """Two mi_ft_micro_step calls at different times into one gradient and one statistics buffer, injected noise, b_global = 2 B,
    accum_steps = 3: each step's out_sample_loss / out_kl, the three statistics rows and the type_out.bias gradient after both against
    the closed forms; every trunk tensor's gradient exactly zero; the head weights' gradients (seeds^T h: the only place the time
    embedding and the trunk show) against float64 oracle autograd."""
    c = _case(shape)
    _offsets(c)
    b_global = 2 * c.B
    grad, stats = torch.zeros_like(c.m.decoder.theta), torch.zeros(3, device="cuda")
    checks, tot = [], None
    names = ["decoder." + k for k in HEADS + ("type_out.bias",)]
    for k, idx in enumerate(idxs):
        nz = R.noise(c.fs, seed=40 + k)
        Lb, KLb = _micro(c, idx, nz, grad, stats, b_global)
        L, KL, st, bias = _closed_form(c, idx, nz, b_global)
        o32, o64 = _oracle(c, idx, nz, torch.float32, b_global), _oracle(c, idx, nz, torch.float64, b_global)
        assert float(KL.min()) > 0.1 and torch.count_nonzero(o32["preds"][0]) == 0 and torch.count_nonzero(o32["preds"][1]) == 0
        checks += [((Lb, L, o32["L"], f"{shape} step {k} L_b"), {}), ((KLb, KL, o32["KL"], f"{shape} step {k} KL_b"), {})]
        new = dict(st=st, st32=o32["stats"].double(), bias=bias, **{n: o64["grads"][n] for n in names[:3]},
                   **{n + "32": o32["grads"][n].double() for n in names})
        tot = new if tot is None else {n: tot[n] + v for n, v in new.items()}
    dev = TA._grads(c.m, grad)
    checks += [((stats[r:r + 1], tot["st"][r:r + 1], tot["st32"][r:r + 1], f"{shape} statistics row {r}"), {}) for r in range(3)]
    checks += [((dev["type_out.bias"], tot["bias"], tot[names[3] + "32"], f"{shape} grad type_out.bias vs sum of seeds"), {})]
    checks += [((dev[n[len("decoder."):]], tot[n], tot[n + "32"], f"{shape} grad {n}"), {}) for n in names[:3]]
    _all(checks)
    TA._assert_trunk_gradient_is_zero(c.m, grad)


# ---- (c) the stacked entry ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("noise", ["injected", "device"])
def test_stacked_micro_steps_with_zero_heads_vs_float64(noise):
    """mi_ft_micro_steps_stacked, 3 replicas of STACK_NA at t = 1, 433, T: statistics and type_out.bias gradient against the sum of three
    closed-form micro-steps -- with injected noise, and with the device's own draws against the host Philox contract: replica j draws at
    call id + j, by the ORIGINAL crystal and atom ids, on a shard with non-zero offsets."""
    from matinvent_amd import finetune
    c = _case("stack")
    idxs, call0, b_global = [T - 1, T - 433, 0], 77, 2 * c.B
    device = noise == "device"
    _offsets(c, *((NODE_OFF, GRAPH_OFF) if device else (0, 0)))
    c.m._noise_calls = call0 - 1
    nzs = [_philox(call0 + j, c.B, c.N) if device else R.noise(c.fs, seed=50 + j) for j in range(3)]
    grad, stats = torch.zeros_like(c.m.decoder.theta), torch.zeros(3, device="cuda")
    try:
        finetune._stacked_micro_steps(c.m, c.prior, c.batch, idxs, None if device else nzs, SIGMA_KL, b_global, ACCUM, grad, stats)
        torch.cuda.synchronize()
    finally:
        _offsets(c)
    assert c.m._noise_calls == call0 + 2
    zs = [tuple(v.double().requires_grad_(device) for v in nz) for nz in nzs]
    forms = [_closed_form(c, idx, z, b_global) for idx, z in zip(idxs, zs)]
    st, bias = sum(f[2] for f in forms), sum(f[3] for f in forms)
    o32 = [_oracle(c, idx, nz, torch.float32, b_global) for idx, nz in zip(idxs, nzs)]
    st32, bias32 = sum(o["stats"] for o in o32), sum(o["grads"]["decoder.type_out.bias"] for o in o32)
    leaves = [v for z in zs for v in z]
    slack = lambda out: _first_order(out, leaves) if device else 0.0
    _all([((stats[r:r + 1], st[r:r + 1], st32[r:r + 1], f"stacked, {noise} noise, statistics row {r}"), dict(slack=slack(st[r:r + 1]))) for r in range(3)]
         + [((TA._grads(c.m, grad)["type_out.bias"], bias, bias32, f"stacked, {noise} noise, grad type_out.bias"), dict(slack=slack(bias)))])
    TA._assert_trunk_gradient_is_zero(c.m, grad)


# ---- (d) non-zero heads: px, pl != 0 in the loops' later trips --------------------------------------------------------------------------

def test_micro_step_with_nonzero_heads_at_86_atoms_vs_float64_oracle():
    """Agent != prior, head_scale = 0.1, na = [86, 3, 1], one micro-step at t = 433: out_sample_loss, out_kl and every gradient tensor
    against the oracle (add_noise + calc_sample_loss + calc_kl_reg + autograd) in float64 on the CPU -- d_x, d_l and the coordinate and
    lattice parts of KL in a second loop trip.  Tolerance: the yardstick's, never looser than tests/test_gpu_train.py's
    test_ft_gradients_and_adam_golden (5e-5 loss, 2e-4 KL, 2e-5 per gradient tensor)."""
    c = _make(HEADS_NA, TA._params(1, seed=7, zero_heads=False)[1], TA._params(1, seed=8, zero_heads=False)[1], seed=23)
    b_global = 2 * c.B
    nz = R.noise(c.fs, seed=60)
    grad, stats = torch.zeros_like(c.m.decoder.theta), torch.zeros(3, device="cuda")
    Lb, KLb = _micro(c, T - 433, nz, grad, stats, b_global)
    o64, o32 = _oracle(c, T - 433, nz, torch.float64, b_global), _oracle(c, T - 433, nz, torch.float32, b_global)
    assert float(o64["preds"][0].abs().max()) > 1e-3 and float(o64["preds"][1].abs().max()) > 1e-3 and float(o64["KL"].min()) > 0
    checks = [((Lb, o64["L"], o32["L"], "non-zero heads L_b"), dict(cap=5e-5)), ((KLb, o64["KL"], o32["KL"], "non-zero heads KL_b"), dict(cap=2e-4))]
    checks += [((stats[r:r + 1], o64["stats"][r:r + 1], o32["stats"][r:r + 1], f"non-zero heads statistics row {r}"), dict(cap=2e-4)) for r in range(3)]
    for k, g in TA._grads(c.m, grad).items():
        assert float(o64["grads"]["decoder." + k].abs().max()) > 0, k
        checks.append(((g, o64["grads"]["decoder." + k], o32["grads"]["decoder." + k], f"non-zero heads grad {k}"), dict(cap=2e-5)))
    _all(checks)

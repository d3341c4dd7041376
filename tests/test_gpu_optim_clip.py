"""GPU checks of global-norm gradient clipping and the non-finite-step guard of the fused Adam (include/matinvent_hip_optim.h,
optim.FusedAdam(max_grad_norm=, skip_nonfinite=), the fine-tune loops' max_grad_norm / skip_nonfinite_steps).

Every reference is float64 torch written here: the norm, torch.nn.utils.clip_grad_norm_'s coefficient min(1, max_norm / (norm + 1e-6)), Adam.

The norm's bound, relative 1e-6, is derived, not measured: the kernel forms every product grad[i] * grad_scale exactly in float64, rounds
each square once (2^-53) and adds in float64 (at most n 2^-53 relative for non-negative terms: 1.4e-9 at the largest n here); the square
root halves that; the one rounding of the norm to float adds 2^-24 = 6e-8.  Nothing is summed in float32 (a strip of S = 0 terms).
No square can overflow or underflow for a finite float gradient; a norm beyond FLT_MAX, like any inf / NaN element, gives a non-finite
norm, and that step is skipped (skip_nonfinite) or applied as it stands -- the same rule as for any other non-finite gradient."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from matinvent_amd import _lib
from matinvent_amd.cspnet import _ptr, _stream
from matinvent_amd.optim import GRAD_STATS, FusedAdam
from tests.optim_clip_util import ft_fixture, ft_step

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
N_BENCH = 12346468                     # the benchmark network's theta
NORM_TOL = 1e-6


def _cap():
    return _lib.load().mi_optim_sweep_elems(1 << 40)      # elements per sweep of the capped grid, from the function that sizes it


def _state():
    return torch.zeros(16, dtype=torch.int32, device="cuda")


def _work(n):
    return torch.empty(_lib.load().mi_optim_workspace_bytes(n) // 4, dtype=torch.float32, device="cuda")


def _grad_norm(g, state, work, max_norm=0.0, skip=0, scale=1.0):
    _lib.check(_lib.load().mi_grad_norm(_ptr(g), g.numel(), scale, max_norm, skip, LR, B1, B2, _ptr(state), _ptr(work), _stream()), "mi_grad_norm")
    return state


def _norm_of(state):
    return state.view(torch.float32)[9]


def _stats(opt):
    return dict(zip(GRAD_STATS, opt.grad_stats().tolist()))


def _gradients(n, seed):
    g = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))
    last = torch.zeros(n, device="cuda")
    last[-1] = -3.25
    return {"normal": g, "normal*1e-20": g * 1e-20, "normal*1e+15": g * 1e15, "one-nonzero-last": last}


def _check_norms(n, seed):
    for what, g in _gradients(n, seed).items():
        ref = g.double().norm()
        assert float(ref) > 0 and bool(torch.isfinite(ref))
        got = _norm_of(_grad_norm(g, _state(), _work(n))).double()
        rel = float((got - ref).abs() / ref)
        print(f"n = {n} {what}: norm {float(got):.9g} ref {float(ref):.17g} rel {rel:.2e}")
        assert rel <= NORM_TOL, (n, what, rel)


def _adam64(p, grads, max_norm=None, lr=LR):
    """float64 Adam (torch.optim.Adam defaults) over the gradients in order, each clipped like clip_grad_norm_ when max_norm is given."""
    p = p.double().clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for s, g in enumerate(grads, 1):
        g = g.double()
        if max_norm is not None:
            g = g * torch.clamp(max_norm / (g.norm() + 1e-6), max=1.0)
        m = B1 * m + (1 - B1) * g
        v = B2 * v + (1 - B2) * g * g
        p = p - lr / (1 - B1 ** s) * m / (v.sqrt() / (1 - B2 ** s) ** 0.5 + EPS)
    return p


@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 100003, "cap-1", "cap", "cap+1"])
def test_norm_and_guarded_step_at_the_sizes_where_indexing_can_go_wrong(n):
    """One element, fewer than a float4, around one block's threads, the existing Adam test's odd size, and exactly / one under / one over
    what the capped grid covers in one sweep: the norm of four kinds of gradient within 1e-6 of float64, and one clipped Adam step within
    2e-6 of float64 on every element (the tail behind the last float4 included)."""
    n = {"cap-1": _cap() - 1, "cap": _cap(), "cap+1": _cap() + 1}.get(n, n)
    _check_norms(n, seed=n % 1000)
    gen = torch.Generator(device="cuda").manual_seed(5)
    p = torch.nn.Parameter(torch.randn(n, device="cuda", generator=gen))
    g = torch.randn(n, device="cuda", generator=gen)
    max_norm = 0.5 * float(g.double().norm())
    ref = _adam64(p.detach(), [g], max_norm)
    p.grad = g.clone()
    opt = FusedAdam([p], lr=LR, max_grad_norm=max_norm)
    opt.step()
    assert float((p.detach().double() - ref).abs().max()) < 2e-6
    s = _stats(opt)
    assert s["applied_steps"] == 1 and s["clipped_steps"] == 1 and abs(s["last_coef"] - 0.5) < 1e-6


def test_norm_at_the_benchmark_size_and_from_an_unaligned_base():
    _check_norms(N_BENCH, seed=7)
    # a gradient that does not start on a 16-byte boundary is read with dword loads: same bound
    n = 100003
    base = torch.randn(n + 1, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))
    g = base[1:]
    assert g.data_ptr() % 16 == 4 and g.is_contiguous()
    got = _norm_of(_grad_norm(g, _state(), _work(n))).double()
    ref = g.double().norm()
    assert float((got - ref).abs() / ref) <= NORM_TOL
    # and the guarded step on unaligned parameters, moments and gradient takes its dword form
    th, m, v = torch.randn(n + 1, device="cuda")[1:], torch.zeros(n + 1, device="cuda")[1:], torch.zeros(n + 1, device="cuda")[1:]
    ref_t = _adam64(th, [g])
    st = _grad_norm(g, _state(), _work(n))
    _lib.check(_lib.load().mi_adam_step_guarded(_ptr(th), _ptr(g), _ptr(m), _ptr(v), n, B1, B2, EPS, 1.0, _ptr(st), _stream()), "mi_adam_step_guarded")
    assert float((th.double() - ref_t).abs().max()) < 2e-6


def test_norm_is_bit_reproducible():
    """The same gradient reduced twice gives the same bits; also after another reduction used the same workspace in between; also on a
    non-default stream."""
    for n in (100003, _cap() + 1):
        gen = torch.Generator(device="cuda").manual_seed(3)
        g, other = torch.randn(n, device="cuda", generator=gen), 7.0 * torch.randn(n, device="cuda", generator=gen)
        work = _work(n)
        a = _norm_of(_grad_norm(g, _state(), work)).clone()
        b = _norm_of(_grad_norm(g, _state(), work)).clone()
        _grad_norm(other, _state(), work)
        c = _norm_of(_grad_norm(g, _state(), work)).clone()
        assert torch.equal(a, b) and torch.equal(a, c) and float(a) > 0
    n = 100003
    g = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    a = _norm_of(_grad_norm(g, _state(), _work(n))).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d = _norm_of(_grad_norm(g, _state(), _work(n))).clone()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(a, d)


def _five_steps(seed=0, n=100003):
    torch.manual_seed(seed)
    p0 = torch.randn(n, device="cuda")
    return p0, [torch.randn(n, device="cuda") for _ in range(5)]


def _run(p0, grads, **kw):
    p = torch.nn.Parameter(p0.clone())
    opt = FusedAdam([p], lr=LR, **kw)
    for g in grads:
        p.grad = g.clone()
        opt.step()
    return p, opt


def test_clipped_adam_matches_float64():
    """test_fused_adam_matches_torch_adam's set-up (100 003 parameters, five steps, lr 1e-3, standard-normal parameters and gradients, its
    2e-6 bound).  max_grad_norm = 1: every step clips (the norm is about 316).  max_grad_norm = 1e30: none does, the coefficient in the
    state block is exactly 1.0, and theta is plain FusedAdam's."""
    p0, grads = _five_steps()
    p, opt = _run(p0, grads, max_grad_norm=1.0)
    assert float((p.detach().double() - _adam64(p0, grads, 1.0)).abs().max()) < 2e-6
    s = _stats(opt)
    assert s["clipped_steps"] == 5 and s["applied_steps"] == 5 and s["skipped_steps"] == 0 and s["nonfinite_steps"] == 0
    norms = [float(g.double().norm()) for g in grads]
    assert abs(s["norm_sum"] - sum(norms)) <= 1e-6 * sum(norms) and abs(s["norm_max"] - max(norms)) <= 1e-6 * max(norms)
    assert abs(s["last_norm"] - norms[-1]) <= 1e-6 * norms[-1] and abs(s["last_coef"] - 1.0 / (norms[-1] + 1e-6)) <= 1e-6 / norms[-1]
    plain, _ = _run(p0, grads)
    p, opt = _run(p0, grads, max_grad_norm=1e30)
    assert float((p.detach() - plain.detach()).abs().max()) < 2e-6
    assert float((p.detach().double() - _adam64(p0, grads)).abs().max()) < 2e-6
    s = _stats(opt)
    assert s["clipped_steps"] == 0 and s["applied_steps"] == 5 and s["last_coef"] == 1.0
    assert opt._opt_state.view(torch.float32)[0].item() == 1.0
    # a statistics reset starts a new period and leaves Adam's own count alone
    opt.grad_stats(reset=True)
    s = _stats(opt)
    assert s["applied_steps"] == 0 and s["norm_sum"] == 0 and s["norm_max"] == 0 and int(opt._opt_state[4]) == 5


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_nonfinite_step_is_skipped_and_does_not_count(bad):
    """Five steps whose third gradient holds one NaN / +inf in its last element (data, not a fault).  skip_nonfinite: theta and both moments
    keep their bits over step 3, the device counts 4 applied / 1 skipped, and the final theta is float64 Adam's over the four finite
    gradients -- which pins the bias corrections to the applied count.  Without the guard the element reaches theta."""
    p0, grads = _five_steps(seed=1)
    grads[2] = grads[2].clone()
    grads[2][-1] = bad
    finite = grads[:2] + grads[3:]
    for kw in (dict(skip_nonfinite=True), dict(skip_nonfinite=True, max_grad_norm=1.0)):
        p = torch.nn.Parameter(p0.clone())
        opt = FusedAdam([p], lr=LR, **kw)
        for i, g in enumerate(grads):
            p.grad = g.clone()
            before = [t.clone() for t in (p.detach(), opt.state[p].get("exp_avg", p0), opt.state[p].get("exp_avg_sq", p0))]
            opt.step()
            if i == 2:
                after = (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])
                assert all(torch.equal(a, b) for a, b in zip(before, after))
                assert int(opt._opt_state[3]) == 0                      # the apply flag
        s = _stats(opt)
        assert s["applied_steps"] == 4 and s["skipped_steps"] == 1 and s["nonfinite_steps"] == 1 and opt.state[p]["step"] == 5
        assert int(opt._opt_state[4]) == 4                              # Adam's count: the applied steps
        assert bool(torch.isfinite(p).all())
        assert float((p.detach().double() - _adam64(p0, finite, kw.get("max_grad_norm"))).abs().max()) < 2e-6
        norms = [float(g.double().norm()) for g in finite]
        assert abs(s["norm_sum"] - sum(norms)) <= 1e-6 * sum(norms)      # the statistics hold the finite norms only
    # neither option: the guarded path does not exist
    p, opt = _run(p0, grads[:2])
    assert not opt.guarded and not hasattr(opt, "_opt_state")
    with pytest.raises(RuntimeError):
        opt.grad_stats()
    # clipping alone does not guard: the NaN (or inf * 0) reaches theta, as with torch's clip_grad_norm_
    p, opt = _run(p0, grads, max_grad_norm=1.0)
    assert bool(torch.isnan(p[-1]))
    s = _stats(opt)
    assert s["applied_steps"] == 5 and s["skipped_steps"] == 0 and s["nonfinite_steps"] == 1


def test_pg_step_clips_like_the_hand_driven_loop():
    """test_pg_step_matches_hand_driven_adam_and_is_deterministic's network, rollout and config, plus max_grad_norm = half of the first
    optimizer step's gradient norm (taken from the unfused reference gradients): pg_step = the hand-driven loop that clips the
    float64-reduced unfused gradient before FusedAdam.step (theta within 1e-6, that test's bound); two calls give the same bits; the epoch
    dicts carry the four statistics, and without the keys exactly today's entries."""
    from oracle import diffcsp_oracle as O
    from matinvent_amd import policy
    from tests.gpu_util import make_module
    from tests.test_gpu_policy_gradient import P_flat, _rollout, _unfused
    hp = O.CSPNetHParams(hidden_dim=64, num_layers=2, num_freqs=8)
    T = 20
    P = O.init_params(hp, seed=9, head_scale=0.1)
    na = [3, 8, 5, 2, 6]
    m0 = make_module(64, 2, 8, T, P)
    _, ro = _rollout(m0, na, seed=41)
    B = ro.num_graphs
    rewards = np.array([0.2, 0.9, 0.5, 0.1, 0.6])
    base = dict(lr=1e-4, epochs=2, timesteps=5, accum_steps=2, clip_range=0.2, adv_clip=5.0, logprob_weights=[1.0, 1.0, 1.0])
    A = torch.from_numpy(policy.advantages(rewards)).cuda()
    M = B * base["accum_steps"]
    w = base["logprob_weights"]
    draws = policy.draw_timesteps(T, B, base["timesteps"], base["epochs"], seed=123)
    first = sum(_unfused(m0, ro, draws[0][k], A, base["clip_range"], w, M)[0] for k in range(base["accum_steps"]))
    max_norm = 0.5 * float(first.double().norm())
    assert max_norm > 0
    cfg = dict(base, max_grad_norm=max_norm)
    runs = []
    for _ in range(2):
        m = make_module(64, 2, 8, T, P)
        stats = policy.pg_step(m, ro, rewards, cfg, seed=123, log=lambda s: None)
        assert len(stats) == 2
        runs.append(m.decoder.theta.detach().clone())
    assert torch.equal(runs[0], runs[1])
    for s in stats:
        assert set(s) == {"loss", "ratio_mean", "approx_kl", "clip_frac", "grad_norm", "grad_norm_max", "clipped_steps", "skipped_steps"}
        assert np.isfinite(list(s.values())).all() and s["skipped_steps"] == 0 and 0 < s["grad_norm"] <= s["grad_norm_max"]
    # by hand
    m = make_module(64, 2, 8, T, P)
    theta = m.decoder.theta
    opt = FusedAdam([theta], lr=cfg["lr"])
    clipped, norms = [0, 0], [[], []]
    for e, dr in enumerate(draws):
        acc = torch.zeros_like(theta)
        for k in range(dr.shape[0]):
            acc += _unfused(m, ro, dr[k], A, cfg["clip_range"], w, M)[0]
            if (k + 1) % cfg["accum_steps"] == 0 or k + 1 == dr.shape[0]:
                norm = acc.double().norm()
                coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
                clipped[e] += int(coef < 1.0)
                norms[e].append(float(norm))
                theta.grad = (acc.double() * coef).float()
                opt.step()
                acc = torch.zeros_like(theta)
    theta.grad = None
    assert (runs[0] - P_flat(m, P)).abs().max().item() > 1e-6
    d = (runs[0] - theta.detach()).abs().max().item()
    assert d <= 1e-6, d
    assert clipped[0] >= 1
    for e in range(2):
        assert stats[e]["clipped_steps"] == clipped[e]
        # (the fused gradient is held to 5e-5 .. 1e-4 of each tensor's largest element by test_gpu_policy_gradient; 1e-3 of the norm leaves room for it)
        assert abs(stats[e]["grad_norm"] - np.mean(norms[e])) <= 1e-3 * np.mean(norms[e])
        assert abs(stats[e]["grad_norm_max"] - max(norms[e])) <= 1e-3 * max(norms[e])
    # without the keys: today's dicts
    m = make_module(64, 2, 8, T, P)
    plain = policy.pg_step(m, ro, rewards, base, seed=123, log=lambda s: None)
    assert all(list(s) == ["loss", "ratio_mean", "approx_kl", "clip_frac"] for s in plain)
    with pytest.raises(ValueError, match="max_grad_norm"):
        policy.pg_step(m, ro, rewards, dict(base, max_grad_norm=0.0), seed=123, log=lambda s: None)


def test_ft_step_clips_the_same_with_one_and_two_groups():
    """With max_grad_norm set, the two-group path (gradients summed before the optimizer step) and the single-group path agree on theta
    within test_ft_step_end_to_end_vs_oracle's tolerance for its grouped cases (1.2e-4 everywhere, 1e-5 on 98 % of the elements) and
    report the same clipped_steps; without the keys the dicts are today's."""
    make_agents, data, rewards, noise_fn, cfg = ft_fixture()
    agent, prior = make_agents()
    probe = ft_step(agent, prior, data, rewards, dict(cfg, max_grad_norm=1e30), noise_fn=noise_fn, fused=True, groups=1, stack=1)
    assert all(s["clipped_steps"] == 0 and s["skipped_steps"] == 0 and s["grad_norm"] > 0 for s in probe)
    max_norm = 0.25 * min(s["grad_norm"] for s in probe)      # a quarter of the mean norm: clips
    out = {}
    for groups in (1, 2):
        agent, prior = make_agents()
        stats = ft_step(agent, prior, data, rewards, dict(cfg, max_grad_norm=max_norm, skip_nonfinite_steps=True), noise_fn=noise_fn, fused=True,
                        groups=groups, stack=1)
        assert all(set(s) == {"loss", "loss_diff", "loss_kl", "grad_norm", "grad_norm_max", "clipped_steps", "skipped_steps"} for s in stats)
        out[groups] = (agent.decoder.theta.detach().clone(), stats)
    d = (out[1][0] - out[2][0]).abs()
    assert float(d.max()) <= 1.2e-4 and float(d.flatten().kthvalue(max(1, int(0.98 * d.numel()))).values) <= 1e-5
    for a, b in zip(out[1][1], out[2][1]):
        assert a["clipped_steps"] == b["clipped_steps"] and a["skipped_steps"] == b["skipped_steps"] == 0
        assert abs(a["grad_norm"] - b["grad_norm"]) <= 1e-3 * a["grad_norm"]
    assert sum(s["clipped_steps"] for s in out[1][1]) >= 1
    agent, prior = make_agents()
    plain = ft_step(agent, prior, data, rewards, cfg, noise_fn=noise_fn, fused=True, groups=1, stack=1)
    assert all(list(s) == ["loss", "loss_diff", "loss_kl"] for s in plain)


WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1])
FORCED = sys.argv[3] == "forced"
if FORCED:
    os.environ["MI_DIST_FORCE_COLLECTIVES"] = "1"     # a world-size-1 group still runs its collectives (matinvent_amd.dist.collectives_on)
import numpy as np, torch, torch.distributed as dist
from tests.optim_clip_util import ft_fixture, ft_step
from matinvent_amd import dist as mdist
torch.cuda.set_device(0)
if FORCED:
    dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
assert mdist.collectives_on() == FORCED
make_agents, data, rewards, noise_fn, cfg = ft_fixture()
agent, prior = make_agents()
probe = ft_step(agent, prior, data, rewards, dict(cfg, max_grad_norm=1e30), noise_fn=noise_fn, fused=True, groups=1, stack=1, log=lambda *_: None)
max_norm = 0.25 * min(s["grad_norm"] for s in probe)      # a quarter of the mean norm: clips
agent, prior = make_agents()
stats = ft_step(agent, prior, data, rewards, dict(cfg, max_grad_norm=max_norm, skip_nonfinite_steps=True), noise_fn=noise_fn, fused=True,
                groups=1, stack=1, log=lambda *_: None)
np.savez(sys.argv[2], theta=agent.decoder.theta.detach().cpu().numpy(), clipped=np.array([s["clipped_steps"] for s in stats]),
         norm=np.array([s["grad_norm"] for s in stats]))
if FORCED:
    dist.barrier(device_ids=[0])
    dist.destroy_process_group()
'''


def test_ft_step_clipping_under_forced_collectives_is_the_plain_run(tmp_path):
    """A world-size-1 RCCL group with forced collectives (the all-reduce in front of every optimizer step, the epoch's statistics in the
    accumulator all-reduce) against the same run without a process group, each in a fresh child process: the same theta bit for bit, the
    same statistics."""
    outs = {}
    for name in ("forced", "plain"):
        script, out_file = tmp_path / f"w_{name}.py", tmp_path / f"w_{name}.npz"
        script.write_text(WORKER)
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29673", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
        env.pop("MI_DIST_FORCE_COLLECTIVES", None)
        r = subprocess.run([sys.executable, str(script), ROOT, str(out_file), name], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        outs[name] = np.load(out_file)
    a, b = outs["forced"], outs["plain"]
    assert np.array_equal(a["theta"], b["theta"])
    assert np.array_equal(a["clipped"], b["clipped"]) and np.array_equal(a["norm"], b["norm"]) and int(a["clipped"].sum()) >= 1

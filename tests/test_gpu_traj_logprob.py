"""GPU checks of DiffCSPModule.forward_logprb (mi_traj_logprob / mi_traj_logprob_backward) and sampling.sample_mdp: parity with the
reference-generated fixture g13, round trips of device-recorded trajectories, parameter gradients against torch autograd through the
oracle, per-crystal timesteps, determinism, stale tapes, and the records sample_mdp hands to forward_logprb."""
import os

import numpy as np
import pytest
import torch

from oracle import diffcsp_oracle as O
from tests.gpu_util import Box, make_module, params_from_golden
from tests.traj_util import STATE_KEYS, forward_logprb as oracle_forward_logprb

pytestmark = pytest.mark.gpu
LP = ("log_prob_l", "log_prob_t", "log_prob_x")


def _rel(a, b, tol, what):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    scale = max(1e-12, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    if os.environ.get("MI_TOL_REPORT"):   # calibration runs: print what was measured next to what is demanded
        print(f"TOL {what}: measured {err / scale:.3e} of max|ref|, demanded {tol:.0e}")
    assert err <= tol * scale, f"{what}: max abs err {err:.3e} > {tol:.0e} * max|ref| ({scale:.3g})"


def _grad_tol(k):
    # as tests/test_gpu_train.py: the time-embedding columns of atom_latent_emb see the device's sin / cos of the pinned table
    return 1e-4 if k == "atom_latent_emb.weight" else 2e-5


def _loss(out, w, v):
    lp_l, lp_t, lp_x, (pl, px, pt) = out
    return (w[0] * lp_l).sum() + (w[1] * lp_t).sum() + (w[2] * lp_x).sum() + (v[0] * pl).sum() + (v[1] * px).sum() + (v[2] * pt).sum()


def _grads(m):
    return {k: m.decoder.theta.grad[o:o + n].view(shape) for k, (o, n, shape) in m.decoder.layout.items()}


def _one_step(m, na, t, seed, step_lr=5e-6):
    """On-distribution state of one reverse step t -> t-1 recorded by the device sampler from a random state at t."""
    gen = torch.Generator().manual_seed(seed)
    B, N = len(na), int(sum(na))
    init = (torch.rand(N, 3, generator=gen), 4 * torch.eye(3) + torch.randn(B, 3, 3, generator=gen), torch.randn(N, 100, generator=gen))
    final, traj = m.sample(Box(na), step_lr=step_lr, seed=seed, init=init, record=True, t_start=t, t_stop=t - 1)
    return _state_of(traj, t, na)


def _state_of(traj, t, na):
    s = {k: traj[t][k].clone() for k in ("atom_types", "frac_coords", "frac_coords_mid", "lattices")}
    s.update(next_atom_types=traj[t - 1]["atom_types"].clone(), next_frac_coords=traj[t - 1]["frac_coords"].clone(),
             next_lattices=traj[t - 1]["lattices"].clone(), num_atoms=torch.as_tensor(na), timesteps=torch.full((len(na),), t, dtype=torch.long))
    return s


def _rand_wv(B, N, seed, dev="cuda"):
    g = torch.Generator().manual_seed(seed)
    w = tuple(torch.randn(B, generator=g).to(dev) for _ in range(3))
    v = (torch.randn(B, 3, 3, generator=g).to(dev), torch.randn(N, 3, generator=g).to(dev), torch.randn(N, 100, generator=g).to(dev))
    return w, v


def _normal_resolution(g, t, P):
    """Per-crystal error model of log_prob_l / log_prob_t: the Normal mean m = c0 (x - c1 pred) of a lattice entry or type logit of
    magnitude |m| is resolved to ulp(|m|) in fp32, and a one-ulp move of m moves log N(x_next; m, sigma) by |x_next - m| / sigma^2 ulp(|m|).
    The reference's chain at T = 20 takes the lattice and the logits to |m| ~ 3e3 (c0 = 100 at t = T), where that is ~1e-3 -- far above
    fp32 round-off of the log-probabilities themselves.  Two ulps per entry, averaged as the log-probabilities are."""
    al, ac, sg = (P[f"beta_scheduler.{k}"].double() for k in ("alphas", "alphas_cumprod", "sigmas"))
    c0, c1, var = 1 / al[t].sqrt(), (1 - al[t]) / (1 - ac[t]).sqrt(), sg[t] ** 2
    out = []
    for x, xn, pr in (("lattices", "next_lattices", "pred_l_pred"), ("atom_types", "next_atom_types", "pred_t_pred")):
        m = c0 * (torch.from_numpy(g[f"t{t}_{x}"]).double() - c1 * torch.from_numpy(g[f"t{t}_{pr}"]).double())
        e = 2 * np.spacing(m.abs().float().numpy()).astype(np.float64) * (torch.from_numpy(g[f"t{t}_{xn}"]).double() - m).abs().numpy() / float(var)
        out.append(e.reshape(len(e), -1).mean(axis=1))
    na = g["num_atoms"]
    off = np.concatenate([[0], np.cumsum(na)])
    return out[0], np.array([out[1][off[b]:off[b + 1]].mean() for b in range(len(na))])


def test_g13_forward_logprb_parity(golden):
    """The reference's own forward_logprb at t = T, T/2, 2 (g13): log-probs within the teacher-forced sampler bound (1e-4) plus the fp32
    resolution of the Normal means (_normal_resolution; measured: 3.0e-4 on log_prob_l at t = 10, every other log-prob <= 1.2e-5), corrector
    predictions within 3e-5 of max|ref| (measured <= 6.4e-7), the accumulated parameter gradients within 5e-5 (see below)."""
    g = golden("g13_forward_logprb")
    P = params_from_golden(g)
    T = int(g["T"])
    m = make_module(64, 2, 8, T, P, sigmas_norm=P["sigma_scheduler.sigmas_norm"])
    m.load_state_dict({k: v for k, v in P.items() if "scheduler" in k}, strict=False)
    m.time_embedding.freqs.copy_(torch.from_numpy(g["time_freqs"]))
    m.decoder.theta.grad = None
    na = g["num_atoms"]
    bad = []

    def check(fn, *a):
        try:
            fn(*a)
        except AssertionError as e:
            bad.append(str(e).splitlines()[0])

    for t in g["ts"]:
        state = {k: torch.from_numpy(g[f"t{t}_{k}"]) for k in STATE_KEYS}
        state.update(num_atoms=torch.from_numpy(na), timesteps=torch.full((len(na),), int(t), dtype=torch.long))
        out = m.forward_logprb(state, step_lr=float(g["step_lr"]))
        res_l, res_t = _normal_resolution(g, int(t), P)
        for i, (k, res) in enumerate(zip(LP, (res_l, res_t, 0.0))):
            ref = g[f"t{t}_{k}"]
            err = np.abs(out[i].detach().cpu().numpy() - ref)
            bound = 1e-4 * np.maximum(1.0, np.abs(ref)) + res
            if os.environ.get("MI_TOL_REPORT"):
                print(f"TOL t={t} {k}: err {np.array2string(err, precision=2, floatmode='unique')} bound {np.array2string(bound, precision=2, floatmode='unique')}")
            if not (err <= bound).all():
                bad.append(f"t={t} {k}: err {err} > bound {bound}")
        for i, k in enumerate(("pred_l_corr", "pred_x_corr", "pred_t_corr")):
            check(_rel, out[3][i], g[f"t{t}_{k}"], 3e-5, f"t={t} {k}")
        w = tuple(torch.from_numpy(g[f"t{t}_w_{k}"]).cuda() for k in "ltx")
        v = tuple(torch.from_numpy(g[f"t{t}_v_{k}"]).cuda() for k in "lxt")
        _loss(out, w, v).backward()
    # the lattice seeds carry the same resolution limit: one ulp of |m| ~ 3e3 against |l_next - m| <= 4.7 at t = 10 is ~5e-5 of the largest seed.
    # Measured on MI355X: <= 2.3e-5 of max|ref| (lattice_out.weight, csp_layer_1.edge_mlp.2.weight), every other tensor <= 2e-5
    for k, gr in _grads(m).items():
        check(_rel, gr, g["G__decoder." + k], max(_grad_tol(k), 5e-5), f"grad {k}")
    assert not bad, "\n".join(bad)


def test_round_trip_of_a_philox_trajectory():
    """Record a Philox chain (8 ragged crystals, T = 50) with the device sampler; forward_logprb at the same weights re-evaluates steps
    t = 50, 25, 2 to the recorded log-probs -- without a tape (no_grad) and with one."""
    hp = O.CSPNetHParams(hidden_dim=64, num_layers=2, num_freqs=8)
    T = 50
    m = make_module(64, 2, 8, T, O.init_params(hp, seed=4, head_scale=0.1))
    na = [1, 3, 5, 8, 2, 12, 4, 7]
    _, traj = m.sample(Box(na), step_lr=5e-6, seed=11, record=True)
    for t in (T, 25, 2):
        state = _state_of(traj, t, na)
        with torch.no_grad():
            out = m.forward_logprb(dict(state), step_lr=5e-6)
        taped = m.forward_logprb(dict(state), step_lr=5e-6)
        for i, k in enumerate(LP):
            rec = traj[t][k].cpu().numpy()
            np.testing.assert_allclose(out[i].cpu().numpy(), rec, rtol=1e-4, atol=1e-4, err_msg=f"{t} {k}")
            np.testing.assert_allclose(taped[i].detach().cpu().numpy(), rec, rtol=1e-4, atol=1e-4, err_msg=f"taped {t} {k}")


@pytest.mark.parametrize("H,L,F,na,T", [(128, 2, 8, [1, 7, 20, 3, 13], 20), (512, 6, 128, [20] * 64, 1000)],
                         ids=["H128-ragged", "benchmark-hparams-64x20"])
def test_gradients_vs_oracle_autograd(H, L, F, na, T):
    """Parameter gradients of sum(w . log-probs) + sum(v . corrector predictions) against torch autograd through the oracle."""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    hp = O.CSPNetHParams(hidden_dim=H, num_layers=L, num_freqs=F)
    P = O.init_params(hp, seed=7, head_scale=0.1)
    m = make_module(H, L, F, T, P)
    B, N = len(na), sum(na)
    t = T // 2 + 3
    state = _one_step(m, na, t, seed=21)
    w, v = _rand_wv(B, N, seed=22)
    m.decoder.theta.grad = None
    out = m.forward_logprb(dict(state), step_lr=5e-6)
    _loss(out, w, v).backward()
    Pg = {k: x.clone().requires_grad_(True) for k, x in P.items()}
    beta = {k: getattr(m.beta_scheduler, k).cpu() for k in ("alphas", "alphas_cumprod", "sigmas")}
    sigma = {k: getattr(m.sigma_scheduler, k).cpu() for k in ("sigmas", "sigmas_norm")}
    cpu_state = {k: x.cpu() for k, x in state.items()}
    ref = oracle_forward_logprb(Pg, hp, beta, sigma, 0.005, cpu_state, 5e-6, m.time_embedding.freqs.cpu())
    _loss(ref, tuple(x.cpu() for x in w), tuple(x.cpu() for x in v)).backward()
    for i, k in enumerate(LP):
        np.testing.assert_allclose(out[i].detach().cpu().numpy(), ref[i].detach().numpy(), rtol=1e-4, atol=1e-4, err_msg=k)
    for k, gr in _grads(m).items():
        _rel(gr, Pg["decoder." + k].grad, _grad_tol(k), f"{H}: grad {k}")


def test_mixed_timesteps_equal_separate_calls():
    """One call with per-crystal timesteps = the calls at each timestep, in log-probs and in summed gradients."""
    hp = O.CSPNetHParams(hidden_dim=64, num_layers=2, num_freqs=8)
    T = 20
    m = make_module(64, 2, 8, T, O.init_params(hp, seed=8, head_scale=0.1))
    na = [4, 9, 2, 6, 5]
    B, N = len(na), sum(na)
    s1, s2 = _one_step(m, na, 17, seed=31), _one_step(m, na, 3, seed=32)
    pick = torch.tensor([b % 2 for b in range(B)], dtype=torch.bool)          # crystal b at t = 3 where pick[b]
    atom = torch.repeat_interleave(pick, torch.tensor(na))
    mixed = {}
    for k in s1:
        if k == "num_atoms":
            mixed[k] = s1[k]
        elif k in ("lattices", "next_lattices", "timesteps"):
            mixed[k] = torch.where(pick.view(-1, *([1] * (s1[k].dim() - 1))).to(s1[k].device), s2[k], s1[k])
        else:
            mixed[k] = torch.where(atom.view(-1, 1).to(s1[k].device), s2[k], s1[k])
    w, v = _rand_wv(B, N, seed=33)
    m.decoder.theta.grad = None
    out = m.forward_logprb(dict(mixed), step_lr=5e-6)
    _loss(out, w, v).backward()
    g_mixed = m.decoder.theta.grad.clone()
    m.decoder.theta.grad = None
    pc, ac = pick.cuda().float(), atom.cuda().float()
    for s, mb, ma in ((s1, 1 - pc, 1 - ac), (s2, pc, ac)):
        o = m.forward_logprb(dict(s), step_lr=5e-6)
        for i in range(3):
            sel = mb.bool()
            np.testing.assert_allclose(out[i][sel].detach().cpu().numpy(), o[i][sel].detach().cpu().numpy(), rtol=1e-5, atol=1e-5)
        _loss(o, tuple(x * mb for x in w), (v[0] * mb.view(-1, 1, 1), v[1] * ma.view(-1, 1), v[2] * ma.view(-1, 1))).backward()
    _rel(g_mixed, m.decoder.theta.grad, 2e-5, "mixed vs separate gradients")


def test_identical_calls_are_bit_identical():
    hp = O.CSPNetHParams(hidden_dim=128, num_layers=2, num_freqs=8)
    m = make_module(128, 2, 8, 20, O.init_params(hp, seed=9, head_scale=0.1))
    na = [20] * 12 + [3, 17]
    state = _one_step(m, na, 12, seed=41)
    w, v = _rand_wv(len(na), sum(na), seed=42)
    res = []
    for _ in range(2):
        m.decoder.theta.grad = None
        out = m.forward_logprb(dict(state), step_lr=5e-6)
        _loss(out, w, v).backward()
        res.append([x.detach().clone() for x in out[:3]] + [x.detach().clone() for x in out[3]] + [m.decoder.theta.grad.clone()])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_stale_tape_raises_and_t1_is_refused():
    from matinvent_amd._lib import MIError
    hp = O.CSPNetHParams(hidden_dim=64, num_layers=2, num_freqs=8)
    m = make_module(64, 2, 8, 20, O.init_params(hp, seed=10, head_scale=0.1))
    na = [3, 6, 4]
    state = _one_step(m, na, 9, seed=51)
    w, v = _rand_wv(len(na), sum(na), seed=52)
    first = m.forward_logprb(dict(state), step_lr=5e-6)
    second = m.forward_logprb(dict(state), step_lr=5e-6)      # same atom counts: the same handle pair, the first call's tapes are gone
    with pytest.raises(MIError, match="overwrote"):
        _loss(first, w, v).backward()
    m.decoder.theta.grad = None
    _loss(second, w, v).backward()
    g_ok = m.decoder.theta.grad.clone()
    assert torch.isfinite(g_ok).all() and g_ok.abs().max() > 0
    # an untaped call in between invalidates a pending tape as well
    third = m.forward_logprb(dict(state), step_lr=5e-6)
    with torch.no_grad():
        m.forward_logprb(dict(state), step_lr=5e-6)
    with pytest.raises(MIError):
        _loss(third, w, v).backward()
    # another atom-count vector uses another handle pair: a pending tape survives it
    fourth = m.forward_logprb(dict(state), step_lr=5e-6)
    m.forward_logprb(dict(_one_step(m, [5, 5], 9, seed=53)), step_lr=5e-6)
    m.decoder.theta.grad = None
    _loss(fourth, w, v).backward()
    assert torch.equal(m.decoder.theta.grad, g_ok)
    bad = dict(state, timesteps=torch.tensor([9, 1, 9]))
    with pytest.raises(ValueError):
        m.forward_logprb(bad, step_lr=5e-6)
    with pytest.raises(ValueError):
        m.forward_logprb(dict(state, timesteps=torch.tensor([21, 9, 9])), step_lr=5e-6)


def test_sample_mdp_records(monkeypatch):
    """sample_mdp keeps exactly the crystals invalid_filter passes, in order; next_* of step t is the state of step t-1; forward_logprb on
    its items reproduces their recorded log-probs."""
    from matinvent_amd import filters, sampling
    hp = O.CSPNetHParams(hidden_dim=64, num_layers=2, num_freqs=8)
    T = 20
    m = make_module(64, 2, 8, T, O.init_params(hp, seed=12, head_scale=0.1))
    np.random.seed(5)
    sample_list, traj = sampling.sample_mdp(8, m, "cuda", seed=3)
    assert len(traj) == T - 1 and [int(s["timesteps"][0]) for s in traj if len(s["timesteps"])] in ([], list(range(T, 1, -1)))
    for d in sample_list:
        g = d.geometry
        assert g["max_cell_edge"] < filters.MAX_CELL_EDGE and g["min_distance"] > filters.MIN_DISTANCE and g["volume"] > filters.MIN_VOLUME

    # a filter that keeps every other crystal: the kept crystals' rows must line up in every record
    real = filters.invalid_filter
    seen = {}

    def alternate(data, sample_struc=None, return_mask=False):
        mask = np.array([i % 2 == 0 for i in range(len(data))])
        seen["data"], seen["mask"] = data, mask
        return mask if return_mask else real(data, sample_struc, return_mask)

    monkeypatch.setattr(filters, "invalid_filter", alternate)
    np.random.seed(6)
    sample_list, traj = sampling.sample_mdp(9, m, "cuda", seed=4)
    kept = [d for d, k in zip(seen["data"], seen["mask"]) if k]
    assert [d.num_atoms for d in sample_list] == [d.num_atoms for d in kept] and len(kept) == 5
    for k, s in enumerate(traj):
        assert s["num_atoms"].tolist() == [d.num_atoms for d in kept]
        assert s["atom_types"].shape[0] == s["frac_coords"].shape[0] == sum(d.num_atoms for d in kept)
        if k + 1 < len(traj):
            nxt = traj[k + 1]
            for a, b in (("next_frac_coords", "frac_coords"), ("next_lattices", "lattices"), ("next_atom_types", "atom_types")):
                assert torch.equal(s[a], nxt[b]), (k, a)
    for s in (traj[0], traj[len(traj) // 2], traj[-1]):
        with torch.no_grad():
            out = m.forward_logprb(dict(s), step_lr=sampling.DEFAULT_STEP_LR["gen"]["mp_20"])
        for i, k in enumerate(LP):
            np.testing.assert_allclose(out[i].cpu().numpy(), s[k].numpy(), rtol=1e-4, atol=1e-4, err_msg=f"{int(s['timesteps'][0])} {k}")

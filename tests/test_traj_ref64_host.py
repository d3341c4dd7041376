"""CPU checks of tests/traj_ref64.py, the float64 yardstick of tests/test_gpu_traj_arithmetic.py: its log-probabilities and their local
derivatives against the float64 oracle (tests/traj_util.forward_logprb on oracle.diffcsp_oracle.cspnet_forward) and its autograd at a
network with non-zero heads, its KL against tests/kl_util, its surrogate against torch autograd, and the states build_state writes:
finite on every element, with the boundary elements where they are meant to be."""
import numpy as np
import pytest
import torch

from oracle import diffcsp_oracle as O
from tests import kl_util, traj_ref64 as R
from tests.traj_util import forward_logprb as oracle_forward_logprb

T = 1000
SIGMA_BEGIN = 0.005
STEP_LR = 5e-6


def _schedules():
    sn = torch.cat([torch.ones(1), torch.linspace(0.6, 1.4, T)])
    return O.beta_tables(T), O.sigma_tables(T, SIGMA_BEGIN, 0.5, sigmas_norm=sn)


def _close(a, b, rtol, what):
    scale = max(1e-300, float(b.abs().max()))
    err = float((a - b).abs().max())
    assert err <= rtol * scale, f"{what}: {err:.3e} > {rtol:.0e} * {scale:.3g}"


def _network(seed=3, L=1):
    hp = O.CSPNetHParams(hidden_dim=64, num_layers=L, num_freqs=8)
    return hp, {k: v.double() for k, v in O.init_params(hp, seed=seed, head_scale=0.3).items()}


def test_logprobs_and_derivatives_match_the_float64_oracle():
    """traj_ref64.logprobs fed the oracle's own predictions = the oracle's three log-probabilities to 1e-12; its derivatives contracted
    with the oracle's d pred / d theta = autograd of the oracle, per parameter tensor."""
    beta, sigma = _schedules()
    b64, s64 = {k: v.double() for k, v in beta.items()}, {k: v.double() for k, v in sigma.items()}
    hp, P = _network()
    na, t = [1, 4, 9, 2], torch.tensor([2, T, 517, 40])
    s = R.step_scalars(beta, sigma, SIGMA_BEGIN, t, STEP_LR)
    state = R.to64(R.build_state(na, t, s, dict(pred_t=torch.randn(100, generator=torch.Generator().manual_seed(1))), seed=5))
    freqs = torch.exp(torch.arange(128, dtype=torch.float64) * -(np.log(10000.0) / 127))
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    ref = oracle_forward_logprb(Pg, hp, b64, s64, SIGMA_BEGIN, state, STEP_LR, freqs)
    pl, pt, pxc, pxp = kl_util.predictions(Pg, hp, state, freqs)
    lp, d = R.logprobs(s, state, (pxc, pl, pxp, pt))
    for k in range(3):
        _close(lp[k].detach(), ref[k].detach(), 1e-12, f"log-prob {k}")
    gen = torch.Generator().manual_seed(2)
    g = [torch.randn(len(na), generator=gen, dtype=torch.float64) for _ in range(3)]
    names = list(Pg)
    g_ref = torch.autograd.grad(sum((g[k] * ref[k]).sum() for k in range(3)), [Pg[k] for k in names], retain_graph=True)
    batch = torch.repeat_interleave(torch.arange(len(na)), torch.tensor(na))
    dl, dt, dxc, dxp = d
    seeds = [g[0][:, None, None] * dl, g[1][batch][:, None] * dt, g[2][batch][:, None] * dxc, g[2][batch][:, None] * dxp]
    g_loc = torch.autograd.grad([pl, pt, pxc, pxp], [Pg[k] for k in names], grad_outputs=seeds, retain_graph=True)
    # ... and autograd through logprobs itself, written in torch
    g_auto = torch.autograd.grad(sum((g[k] * lp[k]).sum() for k in range(3)), [Pg[k] for k in names])
    for k, a, b, c in zip(names, g_loc, g_ref, g_auto):
        assert float(b.abs().max()) > 0, k
        _close(a, b, 1e-9, f"closed-form derivatives x d pred / d theta, {k}")
        _close(c, b, 1e-9, f"autograd through logprobs, {k}")


def test_kl_matches_kl_util():
    beta, sigma = _schedules()
    na, t = [1, 4, 9, 2], torch.tensor([2, T, 517, 40])
    s = R.step_scalars(beta, sigma, SIGMA_BEGIN, t, STEP_LR)
    gen = torch.Generator().manual_seed(4)
    N, B = sum(na), len(na)
    r = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)
    # coordinate heads large enough that some differences of the two means wrap around the cell
    a, p = [(40 * r(N, 3), r(B, 3, 3), 400 * r(N, 3), r(N, 100)) for _ in range(2)]
    val, d = R.kl(s, na, a, p)
    ref = kl_util.kl_terms(s, na, a[1], p[1], a[3], p[3], a[0], p[0], a[2], p[2])
    dref = kl_util.kl_derivatives(s, na, a[1], p[1], a[3], p[3], a[0], p[0], a[2], p[2])
    k = (s["step_pred"] * s["sqrt_sn"])[1] * (a[2] - p[2])[1:5]
    assert float(k.abs().max()) > 0.5          # (wrapped at t = T)
    for i in range(3):
        _close(val[i], ref[i], 1e-12, f"KL term {i}")
    for i in range(4):
        _close(d[i], dref[i], 1e-12, f"KL derivative {i}")


def test_surrogate_gradient_matches_torch_autograd():
    gen = torch.Generator().manual_seed(6)
    B, eps, w, scale = 40, 0.05, (0.5, 1.0, 2.0), 1.0 / 7
    lp_new = torch.randn(3, B, generator=gen, dtype=torch.float64).requires_grad_(True)
    delta = torch.linspace(-3 * eps, 3 * eps, B, dtype=torch.float64)
    lp_old = (lp_new.detach() - delta[None, :] / (3 * torch.tensor(w, dtype=torch.float64)[:, None])).t().contiguous()
    A = torch.randn(B, generator=gen, dtype=torch.float64)
    A[::7] = 0
    L, rho, g, stats = R.surrogate(lp_new.detach(), lp_old, A, eps, w, scale)
    new = (w[0] * lp_new[0] + w[1] * lp_new[1]) + w[2] * lp_new[2]
    old = (w[0] * lp_old[:, 0] + w[1] * lp_old[:, 1]) + w[2] * lp_old[:, 2]
    r = torch.exp(new - old)
    Lt = torch.maximum(-A * r, -A * torch.clamp(r, 1 - eps, 1 + eps))
    (scale * Lt.sum()).backward()
    assert float((rho.log() - delta).abs().max()) < 1e-12
    inside = (rho - 1).abs() <= eps
    assert 0 < int(inside.sum()) < B and torch.equal(stats[3], (~inside).double())
    _close(L, Lt.detach(), 1e-15, "L")
    _close(g, lp_new.grad, 1e-15, "g")
    assert torch.equal(stats[0], L) and torch.equal(stats[1], rho)
    _close(stats[2], 0.5 * delta ** 2, 1e-9, "approx-KL term")
    # clipped where the ratio left the band on the side the advantage does not reward; zero gradient there and at A = 0
    clipped = ((rho > 1 + eps) & (A > 0)) | ((rho < 1 - eps) & (A < 0)) | (A == 0)
    assert torch.equal(g[1] == 0, clipped) and 0 < int(clipped.sum()) < B


@pytest.mark.parametrize("na", [[1, 2, 85, 86, 3, 171], [1, 3, 2] * 100], ids=["crystal-loop-shapes", "grid-shapes"])
def test_built_states_are_finite_on_every_element_and_sit_at_the_boundary(na):
    """The states of the GPU test: |z| <= 3 keeps every wrapped-normal sum far from underflow, so the reference and its derivatives are
    finite on every element (nothing may be left out of a comparison), in float64 and in the float32 formulas; the six forced
    coordinates are exact zeros, exact nextafter(1, 0) and pairs on opposite sides of the boundary within one std of each other."""
    beta, sigma = _schedules()
    B, N = len(na), sum(na)
    t = torch.from_numpy(np.random.default_rng(0).integers(2, T + 1, size=B))
    t[0], t[1] = 2, T
    s = R.step_scalars(beta, sigma, SIGMA_BEGIN, t, STEP_LR)
    bias = torch.randn(100, generator=torch.Generator().manual_seed(1))
    st = R.build_state(na, t, s, dict(pred_t=bias), seed=7)
    for k in ("frac_coords", "frac_coords_mid", "next_frac_coords"):
        assert st[k].dtype == torch.float32 and float(st[k].min()) >= 0 and float(st[k].max()) < 1, k
    lp, d = R.logprobs(s, R.to64(st), R.zero_head_preds(na, bias))
    for v in lp + d:
        assert bool(torch.isfinite(v).all())
    # every nearest-image distance within 3 std (+ the float32 rounding of the coordinates)
    batch = torch.repeat_interleave(torch.arange(B), torch.tensor(na))
    for a, b, std in (("frac_coords_mid", "frac_coords", "std_corr"), ("next_frac_coords", "frac_coords_mid", "std_pred")):
        dist = kl_util.min_image(st[a].double() - st[b].double()).abs() / s[std][batch][:, None]
        assert float(dist.max()) <= 3 + 1e-3, (a, float(dist.max()))
    for a, m, c in (("next_lattices", s["c0"][:, None, None] * st["lattices"].double(), s["sigma"][:, None, None]),
                    ("next_atom_types", (s["c0"][batch][:, None] * (st["atom_types"].double() - s["c1"][batch][:, None] * bias.double())),
                     s["sigma"][batch][:, None])):
        assert float(((st[a].double() - m).abs() / c).max()) <= 3 + 1e-3, a
    x, xm, xn = (st[k].view(-1) for k in ("frac_coords", "frac_coords_mid", "next_frac_coords"))
    i = torch.linspace(0, 3 * N - 1, 6).long().tolist()
    one = R.LAST_BELOW_ONE
    assert float(x[i[0]]) == 0 and float(x[i[1]]) == one and float(xm[i[2]]) == 0 and float(xm[i[3]]) == one
    assert float(xn[i[4]]) == 0 and float(xn[i[5]]) == one
    sc, sp = (s[k][batch][:, None].expand(N, 3).reshape(-1) for k in ("std_corr", "std_pred"))
    for p, q, std, idx in ((x, xm, sc, i[0]), (x, xm, sc, i[1]), (xm, xn, sp, i[2]), (xm, xn, sp, i[3]), (x, xm, sc, i[4]), (x, xm, sc, i[5])):
        assert abs(float(p[idx]) - float(q[idx])) > 0.5, idx                                   # opposite sides of the boundary ...
        assert abs(float(kl_util.min_image(p[idx].double() - q[idx].double()))) <= float(std[idx]) * (1 + 1e-3), idx   # ... one std apart
    # the float32 formulas on the same state: finite too (the yardstick of the device's tolerance is their deviation from float64)
    hp = O.CSPNetHParams(hidden_dim=64, num_layers=1, num_freqs=8)
    P = O.init_params(hp, seed=3)
    for k in ("coord_out.weight", "lattice_out.weight", "type_out.weight"):
        P["decoder." + k] = torch.zeros_like(P["decoder." + k])
    P["decoder.type_out.bias"] = bias
    if N <= 700:
        ref = oracle_forward_logprb(P, hp, beta, sigma, SIGMA_BEGIN, st, STEP_LR)
        for k in range(3):
            assert bool(torch.isfinite(ref[k]).all())
            _close(ref[k].double(), lp[k], 1e-3, f"float32 formulas, log-prob {k}")
        assert torch.count_nonzero(ref[3][0]) == 0 and torch.count_nonzero(ref[3][1]) == 0 and torch.equal(ref[3][2], bias.expand(N, 100))

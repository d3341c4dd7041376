"""CPU checks of tests/ft_ref64.py, the float64 yardstick of tests/test_gpu_ft_arithmetic.py, so that the yardstick is not the code
under test: its noising, sample loss and anchor penalty against oracle.diffcsp_oracle (add_noise, calc_sample_loss, calc_kl_reg) run in
float64 at a network with non-zero heads, its seeds against torch autograd of the reward-weighted total, its statistics against the
expressions finetune accumulates, and the sets build_set writes: the edge values where they are meant to be, every reference output
finite on every element, and the arithmetic facts of the shapes the GPU file runs."""
import numpy as np
import pytest
import torch

from oracle import diffcsp_oracle as O
from tests import ft_ref64 as R

T = 1000
LOOP_NA = [1, 2, 85, 86, 3, 171]
GRID_NA = [1, 3, 2] * 100
STACK_NA = [2, 86, 3]


def _tables():
    sn = torch.cat([torch.ones(1), torch.linspace(0.6, 1.4, T)])
    return dict(alphas_cumprod=O.beta_tables(T)["alphas_cumprod"], **O.sigma_tables(T, 0.005, 0.5, sigmas_norm=sn))


def _close(a, b, rtol, what):
    scale = max(1e-300, float(b.abs().max()))
    err = float((a - b).abs().max())
    assert a.shape == b.shape and err <= rtol * scale, f"{what}: {err:.3e} > {rtol:.0e} * {scale:.3g}"


def _circle(a, b):
    d = (a - b).abs()
    return torch.minimum(d, 1 - d)


def _network(seed, L=1):
    hp = O.CSPNetHParams(hidden_dim=64, num_layers=L, num_freqs=8)
    return hp, O.init_params(hp, seed=seed, head_scale=0.3)


def test_the_shapes_reach_what_they_are_chosen_for():
    assert [3 * n for n in LOOP_NA if 3 * n > 200] == [255, 258, 513]       # 1, 2 and 3 trips of `i += 256`, the last one partial
    assert all(n % 4 for n in LOOP_NA + STACK_NA) and {n % 4 for n in LOOP_NA} == {1, 2, 3}
    B = len(GRID_NA)
    assert 256 < B < 512 and sum(GRID_NA) <= 600 and set(GRID_NA) == {1, 2, 3}   # a second, partial block of the per-crystal fills
    assert 3 * 86 > 256 and 3 * len(STACK_NA) > len(STACK_NA)                 # the stacked case: a second trip inside every replica


@pytest.mark.parametrize("times", [[1] * 5, [T] * 5, [433] * 5, [1, T, 2, 517, 999]], ids=["t=1", "t=T", "t=433", "per-crystal"])
def test_noising_loss_and_kl_match_the_float64_oracle(times):
    """ft_ref64.add_noise / loss_kl / stats fed the oracle's own predictions = the oracle run in float64, to 1e-12 (in_frac on the circle)."""
    tables = _tables()
    na = [1, 4, 9, 2, 86]
    fs = R.build_set(na, seed=3)
    nz = R.noise(fs, seed=4)
    (hp, P), (_, Q) = _network(3), _network(4)
    scalar = len(set(times)) == 1
    o = R.oracle_micro_step(hp, P, Q, tables, fs, nz, torch.float64, time_idx=T - times[0] if scalar else None, times=None if scalar else times,
                            sigma=0.025, b_global=2 * len(na), accum=3)
    ref = R.add_noise(fs, R.schedule(tables, times), nz)
    for k, v in zip(("in_types", "in_lat", "rand_l", "tar_x", "rand_t"), o["noised"][::2] + o["targets"]):
        _close(ref[k], v, 1e-12, k)
    assert float(_circle(ref["in_frac"], o["noised"][1]).max()) <= 1e-12
    _close(R.lattice_matrix(fs["lengths"], fs["angles"]), O.lattice_params_to_matrix(fs["lengths"].double(), fs["angles"].double()), 1e-15, "lattice")
    L, KL = R.loss_kl(o["preds"], o["prior_preds"], (ref["rand_l"], ref["tar_x"], ref["rand_t"]), R.COSTS, na)
    _close(L, o["L"], 1e-12, "L_b")
    _close(KL, o["KL"], 1e-12, "KL_b")
    assert float(KL.min()) > 0
    st = R.stats(L, KL, fs["reward"], 0.025, 2 * len(na))
    _close(st, o["stats"], 1e-12, "statistics rows")


def test_seeds_match_torch_autograd():
    """ft_ref64.seeds = autograd of (r L + sigma (1.1 - r) KL).sum() / (b_global accum) with respect to the agent's predictions, with
    rewards 0, 1 and 1.1 among the crystals; contracted with d pred / d theta they are the oracle's parameter gradients."""
    na = [1, 2, 86, 3, 5]
    B, N = len(na), sum(na)
    fs = R.build_set(na, seed=5)
    gen = torch.Generator().manual_seed(6)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    pa = tuple(v.requires_grad_(True) for v in (r(B, 3, 3), r(N, 3), r(N, 100)))
    pp, tg = (r(B, 3, 3), r(N, 3), r(N, 100)), (r(B, 3, 3), r(N, 3), r(N, 100))
    sigma, b_global, accum = 0.025, 2 * B, 3
    L, KL = R.loss_kl(pa, pp, tg, R.COSTS, na)
    rw = fs["reward"].double()
    assert rw[:3].tolist() == [0.0, 1.0, float(np.float32(1.1))]
    total = (rw * L + sigma * (1.1 - rw) * KL).sum() / (b_global * accum)
    auto = torch.autograd.grad(total, pa)
    closed = R.seeds(tuple(v.detach() for v in pa), pp, tg, R.COSTS, na, fs["reward"], sigma, b_global, accum)
    for a, b, k in zip(closed, auto, ("d_l", "d_x", "d_t")):
        assert float(b.abs().max()) > 0
        _close(a, b, 1e-13, k)
    # crystal 0 (r = 0): only the anchor term; crystal 2 (r = 1.1 in float32): the anchor term's weight is round-off
    assert torch.equal(closed[0][0], sigma * 1.1 / (b_global * accum) * 2 * (pa[0][0].detach() - pp[0][0]) / 9)
    _close(closed[0][2], rw[2] / (b_global * accum) * R.COSTS[0] * 2 * (pa[0][2].detach() - tg[0][2]) / 9, 1e-6, "d_l at r = 1.1")


def test_seeds_contracted_with_the_network_are_the_oracles_gradients():
    tables = _tables()
    na = [3, 86, 1]
    fs = R.build_set(na, seed=7)
    nz = R.noise(fs, seed=8)
    (hp, P), (_, Q) = _network(5), _network(6)
    kw = dict(time_idx=600, sigma=0.025, b_global=2 * len(na), accum=3)
    o = R.oracle_micro_step(hp, P, Q, tables, fs, nz, torch.float64, grad=True, **kw)
    n2g = torch.repeat_interleave(torch.arange(len(na)), torch.tensor(na))
    it, fr, lat = o["noised"]
    Pg = {k: v.double().requires_grad_(True) for k, v in P.items()}
    pa = O.cspnet_forward(Pg, hp, o["t_emb"], it, fr, lat, torch.tensor(na), n2g)
    sd = R.seeds(tuple(v.detach() for v in pa), o["prior_preds"], o["targets"], R.COSTS, na, fs["reward"], 0.025, 2 * len(na), 3)
    names = list(Pg)
    g = torch.autograd.grad(pa, [Pg[k] for k in names], grad_outputs=sd)
    for k, a in zip(names, g):
        assert float(o["grads"][k].abs().max()) > 0, k
        _close(a, o["grads"][k], 1e-9, f"seeds x d pred / d theta, {k}")


@pytest.mark.parametrize("na", [LOOP_NA, GRID_NA, STACK_NA, [86, 3, 1]], ids=["crystal-loop-shapes", "grid-shapes", "stack-shapes", "non-zero-heads-shapes"])
def test_built_sets_hold_the_edge_values_and_every_reference_output_is_finite(na):
    """The sets of the GPU test: the edge values are where build_set says, the paired noise crosses the cell boundary at the smallest and
    at the largest sigma, and the reference (and the float32 formulas on the same inputs) are finite on every element at t = 1, t = T and
    in between -- nothing may be left out of a comparison."""
    tables = _tables()
    B, N = len(na), sum(na)
    fs = R.build_set(na, seed=11)
    nz = R.noise(fs, seed=12)
    x = fs["frac_coords"].view(-1)
    off = np.concatenate([[0], np.cumsum(na)])
    assert fs["frac_coords"].dtype == torch.float32 and float(x.min()) == 0 and float(x.max()) == R.LAST_BELOW_ONE
    for b in range(B):
        assert float(x[3 * off[b]]) == 0 and float(x[3 * off[b + 1] - 1]) == R.LAST_BELOW_ONE
    assert fs["angles"][0].tolist() == [90.0] * 3 and fs["angles"][1].tolist() == [60.0] * 3
    assert 4 <= float(fs["lengths"].min()) and float(fs["lengths"].max()) <= 10
    assert int(fs["atom_types"][0]) == 1 and int(fs["atom_types"][-1]) == 100 and int(fs["atom_types"].min()) >= 1 and int(fs["atom_types"].max()) <= 100
    assert fs["reward"][:3].tolist() == [0.0, 1.0, float(np.float32(1.1))] and float(fs["reward"].max()) == float(np.float32(1.1))
    assert float(np.cos(np.float32(90.0) * np.float32(0.017453292519943295), dtype=np.float32)) != 0    # (why 90 degrees is an edge value)
    idx, sign = fs["boundary"]
    bias_a, bias_p = (torch.randn(100, generator=torch.Generator().manual_seed(s)) for s in (1, 2))
    for times in ([1] * B, [T] * B, [433] * B, np.random.default_rng(0).integers(1, T + 1, size=B).tolist()):
        sched = R.schedule(tables, times)
        out = R.add_noise(fs, sched, nz)
        moved = fs["frac_coords"].double().view(-1)[idx] + (sched[:, 2][R._batch(na)[1]][:, None] * nz[1].double()).view(-1)[idx]
        assert bool(((moved < 0) == (sign < 0)).all()) and bool(((moved >= 1) == (sign > 0)).all())     # every boundary coordinate crosses
        tg = (out["rand_l"], out["tar_x"], out["rand_t"])
        pa, pp = R.zero_head_preds(na, bias_a), R.zero_head_preds(na, bias_p)
        L, KL = R.loss_kl(pa, pp, tg, R.COSTS, na)
        sd = R.seeds(pa, pp, tg, R.COSTS, na, fs["reward"], 0.025, 2 * B, 3)
        st = R.stats(L, KL, fs["reward"], 0.025, 2 * B)
        for v in list(out.values()) + [L, KL, st] + list(sd):
            assert bool(torch.isfinite(v).all())
        assert float(out["in_frac"].min()) >= 0 and float(out["in_frac"].max()) < 1
        _close(KL, ((bias_a.double() - bias_p.double()) ** 2).mean().expand(B), 1e-14, "zero heads: KL_b is one constant")
        # the float32 formulas (the oracle's add_noise in float32): finite too, and close
        n32 = R.oracle_add_noise(tables, fs, nz, torch.float32, times=times)
        for v in n32[0][1:4] + n32[1]:
            assert bool(torch.isfinite(v).all())
        _close(n32[1][1].double(), out["tar_x"], 1e-4, "float32 formulas, tar_x")
        _close(n32[0][3].double(), out["in_lat"], 1e-5, "float32 formulas, in_lat")

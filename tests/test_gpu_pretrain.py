"""GPU checks of supervised denoising training (matinvent_amd/csrc/pretrain.hip under mi_pretrain_micro_step; matinvent_amd.pretrain;
DiffCSPModule.training_step; pipeline.Pretrain) against tests/pretrain_ref64.py and the oracle.

(1) The loss, seeds and statistics kernels with the network taken out: zero head weights (predictions exactly 0, 0, type_out.bias), sets
of tests/ft_ref64.build_set at LOOP_NA = [1, 2, 85, 86, 3, 171] (3n = 255, 258, 513: one, two and three trips of the 256-thread loops,
the last partial) and at [1, 3, 2] x 100 (300 crystals: a second, partial block of the time gather, the stats kernel's loop), mixed
times that include t = 1 and t = T.  Tolerance: DESIGN 25's rule as tests/test_gpu_ft_arithmetic._check implements it -- 4 x the float32
CPU formulas' own deviation from float64, relative to max|ref64|, floor 4 * 2^-24.  The noise is injected, so no Philox slack enters.
(2)-(5) With heads, H = 64, L = 2, F = 8, perturbed LayerNorm parameters: every gradient tensor within 2e-5 of max|ref| and the
statistics within 1e-4 relative (the bounds of tests/test_gpu_train._grad_case and of its loss checks) of float32 oracle autograd.
(6)-(10) fit against the oracle's literal loop, repeatability, learning, the drop-in round trip, and device memory over many
mini-batches of distinct atom counts."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tests.test_gpu_traj_arithmetic as TA
from oracle import diffcsp_oracle as O
from tests import ft_ref64 as R
from tests import pretrain_ref64 as PR
from tests.gpu_util import make_module
from tests.test_gpu_ft_arithmetic import _all, _tables
from tests.test_gpu_train import _rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T = 1000
LOOP_NA = [1, 2, 85, 86, 3, 171]
GRID_NA = [1, 3, 2] * 100
SEED = 1234
ACCUM = 3
HP = O.CSPNetHParams(hidden_dim=64, num_layers=2, num_freqs=8)


def test_the_shapes_reach_what_they_are_chosen_for():
    assert [3 * n for n in LOOP_NA if 3 * n > 200] == [255, 258, 513] and max(LOOP_NA) == 171 and min(LOOP_NA) == 1
    assert 256 < len(GRID_NA) < 512 and len(GRID_NA) % 256 != 0
    assert {1, T} <= set(_times("loop", 0).tolist()) and {1, T} <= set(_times("grid", 0).tolist())


def _ns(fs):
    return SimpleNamespace(**{k: fs[k] for k in R.SET_KEYS})


def _times(shape, k):
    if shape == "loop":
        return np.array([[1, T, 433, 2, T, 517], [T, 1, 7, 999, 250, 1]][k], dtype=np.int32)
    t = np.random.default_rng(k).integers(1, T + 1, size=len(GRID_NA)).astype(np.int32)
    t[0], t[1], t[-1] = 1, T, T
    return t


# ---- (1) zero heads -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _zero_case(shape):
    na = LOOP_NA if shape == "loop" else GRID_NA
    hp, P = TA._params(1, seed=3)
    c = SimpleNamespace(hp=hp, P=P, na=na, B=len(na), N=sum(na), m=TA._module(1, P), fs=R.build_set(na, seed=21), bias=P["decoder.type_out.bias"])
    c.tables, c.freqs = _tables(c.m), c.m.time_embedding.freqs.cpu()
    return c


@pytest.mark.parametrize("shape", ["loop", "grid"])
def test_loss_seeds_and_statistics_with_zero_heads_vs_float64(shape):
    """Two micro-steps at different mixed times into one gradient and one statistics buffer, b_global = 2 B + 1, n_global = N + 11,
    accum_steps = 3: the four statistics, each step's out_parts, the type_out.bias gradient (the column sums of the type seeds) against
    the closed forms; the head weights' gradients (seeds^T h: where the per-crystal time embedding shows) against float64 oracle
    autograd; every trunk tensor's gradient exactly zero."""
    from matinvent_amd import pretrain
    c = _zero_case(shape)
    bg, ng = 2 * c.B + 1, c.N + 11
    grad, stats = torch.zeros_like(c.m.decoder.theta), torch.zeros(4, device="cuda")
    names = ["decoder." + k for k in TA.HEADS + ("type_out.bias",)]
    checks, tot = [], None
    for k in range(2):
        times, nz = _times(shape, k), R.noise(c.fs, seed=40 + k)
        parts = torch.full((c.B, 3), float("nan"), device="cuda")
        pretrain.train_step(c.m, _ns(c.fs), times, noise=nz, grad=grad, stats=stats, b_global=bg, n_global=ng, accum_steps=ACCUM, out_parts=parts)
        out = R.add_noise(c.fs, R.schedule(c.tables, times), nz)
        preds, tg = R.zero_head_preds(c.na, c.bias), (out["rand_l"], out["tar_x"], out["rand_t"])
        kw = dict(b_global=bg, n_global=ng, accum=ACCUM, freqs=c.freqs, grad=True)
        o32 = PR.oracle_training_step(c.hp, c.P, c.tables, c.fs, nz, torch.float32, times, **kw)
        o64 = PR.oracle_training_step(c.hp, c.P, c.tables, c.fs, nz, torch.float64, times, **kw)
        assert torch.count_nonzero(o32["preds"][0]) == 0 and torch.count_nonzero(o32["preds"][1]) == 0
        ref_parts = PR.parts(preds, tg, c.na)
        for j, what in enumerate(("lattice", "coord", "type")):
            checks.append(((parts[:, j], ref_parts[:, j], o32["parts"][:, j], f"{shape} step {k} out_parts {what}"), {}))
        new = dict(st=PR.stats(preds, tg, PR.COSTS, bg, ng), st32=o32["stats"].double(), bias=PR.seeds(preds, tg, PR.COSTS, bg, ng, ACCUM)[2].sum(dim=0),
                   **{n: o64["grads"][n] for n in names[:3]}, **{n + "32": o32["grads"][n].double() for n in names})
        tot = new if tot is None else {n: tot[n] + v for n, v in new.items()}
    dev = TA._grads(c.m, grad)
    checks += [((stats[r:r + 1], tot["st"][r:r + 1], tot["st32"][r:r + 1], f"{shape} statistics {PR.STATS[r]}"), {}) for r in range(4)]
    checks += [((dev["type_out.bias"], tot["bias"], tot[names[3] + "32"], f"{shape} grad type_out.bias vs the column sums of the type seeds"), {})]
    checks += [((dev[n[len("decoder."):]], tot[n], tot[n + "32"], f"{shape} grad {n}"), {}) for n in names[:3]]
    _all(checks)
    TA._assert_trunk_gradient_is_zero(c.m, grad)
    if shape == "loop":   # what a per-crystal-mean loss would have given for the coordinate part: far outside any tolerance above
        per_crystal = float(R.loss_kl(preds, preds, tg, (0.0, 1.0, 0.0), c.na)[0].sum() / bg)
        assert abs(per_crystal - float(PR.stats(preds, tg, (0.0, 1.0, 0.0), bg, ng)[0])) > 1e-3 * per_crystal


# ---- (2)-(5) with heads ---------------------------------------------------------------------------------------------------------------

def _params(seed=5):
    P = O.init_params(HP, seed=seed)
    gen = torch.Generator().manual_seed(seed + 100)
    for k in P:
        if "layer_norm" in k:
            P[k] = P[k] + 0.1 * torch.randn(P[k].shape, generator=gen)
    return P


def _sigmas_norm():
    return torch.cat([torch.ones(1), 0.5 + torch.rand(T, generator=torch.Generator().manual_seed(9))])


@functools.lru_cache(maxsize=None)
def _heads_case(na):
    P = _params()
    c = SimpleNamespace(P=P, na=list(na), B=len(na), N=sum(na), m=make_module(64, 2, 8, T, P, sigmas_norm=_sigmas_norm()), fs=R.build_set(list(na), seed=23))
    c.tables, c.freqs = _tables(c.m), c.m.time_embedding.freqs.cpu()
    c.times = np.random.default_rng(len(na)).integers(1, T + 1, size=c.B).astype(np.int32)
    c.times[0], c.times[1] = 1, T
    c.nz = R.noise(c.fs, seed=60)
    c.ref = PR.oracle_training_step(HP, P, c.tables, c.fs, c.nz, torch.float32, c.times, freqs=c.freqs, grad=True)   # computed once, left unchanged
    return c


def _grads_close(m, flat, ref, what, tol=2e-5):
    for k, g in TA._grads(m, flat).items():
        _rel(g, ref["decoder." + k], tol, f"{what}: grad {k}")


def _stats_close(stats, ref, what, tol=1e-4):
    for r, name in enumerate(PR.STATS):
        assert abs(float(stats[r]) - float(ref[r])) <= tol * abs(float(ref[r])), f"{what}: {name} {float(stats[r])} vs {float(ref[r])}"


NA_A, NA_B, NA_C = (4, 2, 6, 3), (1, 7, 20, 3, 13), (3, 5, 2)


@pytest.mark.parametrize("na", [NA_A, NA_B], ids=["4-2-6-3", "1-7-20-3-13"])
def test_gradients_with_heads_vs_oracle_autograd(na):
    """Per-crystal times, injected noise, costs (1, 1, 20): every parameter tensor of the fused entry AND of training_step + autograd
    within 2e-5 of max|ref|, the four statistics within 1e-4 relative."""
    from matinvent_amd import pretrain
    c = _heads_case(na)
    assert (c.m.cost_lattice, c.m.cost_coord, c.m.cost_type) == (1.0, 1.0, 20.0)
    grad, stats = torch.zeros_like(c.m.decoder.theta), torch.zeros(4, device="cuda")
    pretrain.train_step(c.m, _ns(c.fs), c.times, noise=c.nz, grad=grad, stats=stats)
    _grads_close(c.m, grad, c.ref["grads"], "fused")
    _stats_close(stats, c.ref["stats"], "fused")
    c.m.decoder.theta.grad = None
    loss, d = c.m.training_step(_ns(c.fs), times=c.times, noise=c.nz)
    assert list(d) == list(PR.STATS) and d["loss"] is loss
    loss.backward()
    _grads_close(c.m, c.m.decoder.theta.grad, c.ref["grads"], "training_step")
    _stats_close(torch.stack([d[k].detach() for k in PR.STATS]), c.ref["stats"], "training_step")
    c.m.decoder.theta.grad = None


def test_shards_with_device_noise_sum_to_the_unsplit_call():
    """[1, 7, 20, 3, 13] as handles of [1, 7] and [20, 3, 13] with their node / graph offsets and the whole batch's b_global, n_global,
    the device's Philox noise at one call id: summed gradients and statistics equal the unsplit call's; the shards' per-crystal sums are
    the whole batch's rows (their draws are the whole batch's)."""
    from matinvent_amd import pretrain
    c = _heads_case(NA_B)
    kw = dict(seed=SEED, call_id=17, b_global=c.B, n_global=c.N)
    g0, s0, p0 = torch.zeros_like(c.m.decoder.theta), torch.zeros(4, device="cuda"), torch.zeros(c.B, 3, device="cuda")
    pretrain.train_step(c.m, _ns(c.fs), c.times, grad=g0, stats=s0, out_parts=p0, **kw)
    g1, s1 = torch.zeros_like(g0), torch.zeros(4, device="cuda")
    ps = []
    for idx, offsets in (([0, 1], (0, 0)), ([2, 3, 4], (8, 2))):
        ps.append(torch.zeros(len(idx), 3, device="cuda"))
        pretrain.train_step(c.m, _ns(PR.subset(c.fs, idx)), c.times[idx], grad=g1, stats=s1, out_parts=ps[-1], offsets=offsets, **kw)
    assert float(s0[0]) > 0 and float(g0.abs().max()) > 0
    _grads_close(c.m, g1, {"decoder." + k: v.cpu() for k, v in TA._grads(c.m, g0).items()}, "shards")
    _stats_close(s1, s0, "shards")
    _rel(torch.cat(ps), p0.cpu(), 1e-5, "the shards' per-crystal sums")
    # ... and without the offsets the second shard draws other noise: the check above can fail
    q = torch.zeros(3, 3, device="cuda")
    pretrain.train_step(c.m, _ns(PR.subset(c.fs, [2, 3, 4])), c.times[[2, 3, 4]], forward_only=True, out_parts=q, **kw)
    assert float((q - p0[2:]).abs().max()) > 1e-3 * float(p0[2:].abs().max())


def test_forward_only_changes_nothing_and_agrees_with_the_taped_call():
    """grad_theta = NULL behind one optimizer step (so that Adam's moments exist): theta, theta.grad and the moments keep their bits; the
    four statistics are the taped call's within 1e-4 relative."""
    from matinvent_amd import pretrain
    from matinvent_amd.optim import FusedAdam
    c = _heads_case(NA_A)
    m = make_module(64, 2, 8, T, c.P, sigmas_norm=_sigmas_norm())
    opt = FusedAdam([m.decoder.theta], lr=1e-4)
    pretrain.train_step(m, _ns(c.fs), c.times, noise=c.nz)
    opt.step()
    opt.zero_grad(set_to_none=False)
    taped = pretrain.train_step(m, _ns(c.fs), c.times, noise=c.nz)
    torch.cuda.synchronize()
    st = opt.state[m.decoder.theta]
    live = (m.decoder.theta, m.decoder.theta.grad, st["exp_avg"], st["exp_avg_sq"])
    before = [v.detach().clone() for v in live]
    assert float(before[1].abs().max()) > 0 and float(before[2].abs().max()) > 0
    parts = torch.zeros(c.B, 3, device="cuda")
    fwd = pretrain.train_step(m, _ns(c.fs), c.times, noise=c.nz, forward_only=True, out_parts=parts)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(live, before)) and st["step"] == 1
    _stats_close(fwd, taped, "forward-only vs taped")
    assert float(parts.min()) > 0


def test_accum_steps_3_over_three_mini_batches_is_the_scaled_sum_of_three_calls():
    from matinvent_amd import pretrain
    cs = [_heads_case(na) for na in (NA_A, NA_B, NA_C)]
    m = cs[0].m
    G, parts = torch.zeros_like(m.decoder.theta), []
    for c in cs:
        pretrain.train_step(m, _ns(c.fs), c.times, noise=c.nz, grad=G, accum_steps=3)
        parts.append(torch.zeros_like(G))
        pretrain.train_step(m, _ns(c.fs), c.times, noise=c.nz, grad=parts[-1], accum_steps=1)
    want = (parts[0] + parts[1] + parts[2]) / 3
    _grads_close(m, G, {"decoder." + k: v.cpu() for k, v in TA._grads(m, want).items()}, "accum_steps = 3")


# ---- (6)-(8) fit ----------------------------------------------------------------------------------------------------------------------

FIT_NA = [4, 2, 6, 3, 1, 7]


def _fit_set(seed=11):
    from matinvent_amd.data import CrystalData
    fs = R.build_set(FIT_NA, seed=seed)
    off = np.concatenate([[0], np.cumsum(FIT_NA)])
    data = [CrystalData(fs["frac_coords"][off[i]:off[i + 1]], fs["atom_types"][off[i]:off[i + 1]], fs["lengths"][i:i + 1], fs["angles"][i:i + 1])
            for i in range(len(FIT_NA))]
    return fs, data


def test_fit_vs_the_oracles_literal_loop():
    """6 crystals, batch_size 3, 2 epochs, lr 1e-4: 4 Adam steps; injected noise, the plan and the times of batch_plan / draw_times.
    Bounds of tests/test_gpu_train.test_ft_step_end_to_end_vs_oracle: every parameter within 1.2e-4, the 98th percentile of the
    differences within 1e-5, each logged loss within 1e-4 max(1, |ref|)."""
    from matinvent_amd import pretrain
    P0 = O.init_params(HP, seed=3)
    gen = torch.Generator().manual_seed(9)
    for k in P0:
        P0[k] = P0[k] + 0.01 * torch.randn(P0[k].shape, generator=gen)
    m = make_module(64, 2, 8, T, P0, sigmas_norm=_sigmas_norm())
    fs, data = _fit_set()
    plans = {e: pretrain.batch_plan(6, 3, e, SEED) for e in range(2)}
    assert all(len(p) == 2 for p in plans.values())
    noises = {}
    for e, plan in plans.items():
        for s, idx in enumerate(plan):
            B, N = len(idx), sum(FIT_NA[i] for i in idx)
            noises[(e, s)] = (torch.randn(B, 3, 3, generator=gen), torch.randn(N, 3, generator=gen), torch.randn(N, 100, generator=gen))
    stats = pretrain.fit(m, data, dict(lr=1e-4, epochs=2, batch_size=3), seed=SEED, noise_fn=lambda e, s: noises[(e, s)], log=lambda *_: None)
    A, logged = PR.oracle_fit(HP, P0, _tables(m), {k: fs[k] for k in R.SET_KEYS}, lambda e: plans[e],
                              lambda e, s, B: pretrain.draw_times(B, T, e, s, SEED), lambda e, s: noises[(e, s)], 2, 1e-4,
                              freqs=m.time_embedding.freqs.cpu())
    assert m._noise_calls == 4 and len(stats) == 2 and all(d["lr"] == 1e-4 for d in stats)
    moved = max(float((w.detach().cpu() - P0["decoder." + k]).abs().max()) for k, w in m.decoder.views().items())
    assert 1e-4 < moved < 1e-3   # (4 Adam steps of lr = 1e-4)
    for k, w in m.decoder.views().items():
        d = (w.detach().cpu() - A["decoder." + k]).abs()
        assert float(d.max()) <= 1.2e-4, f"{k}: {float(d.max())}"
        assert float(d.flatten().kthvalue(max(1, int(0.98 * d.numel()))).values) <= 1e-5, k
    for e in range(2):
        for key, ref in zip(("train_loss", "lattice_loss", "coord_loss", "type_loss"), logged[e]):
            assert abs(stats[e][key] - ref) <= 1e-4 * max(1.0, abs(ref)), (e, key, stats[e][key], ref)


def test_two_fit_runs_with_one_seed_give_the_same_weights():
    """Device noise, shuffled plan, accum_steps 2, a validation set, clipping on: torch.equal weights, equal epoch dicts."""
    from matinvent_amd import pretrain
    _, data = _fit_set()
    _, val = _fit_set(seed=12)
    cfg = dict(lr=1e-3, epochs=2, batch_size=2, accum_steps=2, max_grad_norm=1.0)
    runs = []
    for _ in range(2):
        m = make_module(64, 2, 8, T, _params(), sigmas_norm=_sigmas_norm())
        stats = pretrain.fit(m, data, cfg, val_list=val[:4], seed=SEED, log=lambda *_: None)
        runs.append((m.decoder.theta.detach().clone(), stats))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    d = runs[0][1][0]
    assert {"train_loss", "val_loss", "val_type_loss", "lr", "grad_norm", "clipped_steps"} <= set(d) and np.isfinite(list(d.values())).all()
    assert d["val_loss"] > 0 and d["val_loss"] != runs[0][1][1]["val_loss"]
    # evaluate: the same set through mini-batches of 1 and of 4 crystals is the same number up to summation order
    m = make_module(64, 2, 8, T, _params(), sigmas_norm=_sigmas_norm())
    e1, e4 = pretrain.evaluate(m, val, 1, seed=SEED), pretrain.evaluate(m, val, 4, seed=SEED)
    for k in PR.STATS:
        assert abs(e1[k] - e4[k]) <= 2e-5 * abs(e4[k]), (k, e1[k], e4[k])
    at_k = pretrain.evaluate(m, val, 4, seed=SEED, times=T)
    assert at_k["loss"] > 0 and at_k["loss"] != e4["loss"]


def test_it_learns():
    """The same 6 crystals as every mini-batch, the shipped sigmas_norm table, 4 fixed (times, noise) pairs reused every epoch, 12
    epochs at lr 1e-3 from the oracle's seed-3 weights: the device's last-epoch train_loss must lie below the midpoint of the oracle's
    first- and last-epoch losses (the oracle's own loop, run here on the CPU, goes 34.6 -> 18.9 with all three parts falling)."""
    from matinvent_amd import pretrain
    P0 = O.init_params(HP, seed=3)
    sn = torch.from_numpy(np.load(os.path.join(ROOT, "matinvent_amd", "data", "sigmas_norm_T1000_b0.005_e0.5_seed1234.npy"))).float()
    m = make_module(64, 2, 8, T, P0, sigmas_norm=sn)
    fs, data = _fit_set()
    gen = torch.Generator().manual_seed(5)
    pairs = [(torch.randint(1, T + 1, (6,), generator=gen).numpy(), R.noise(fs, seed=70 + k)) for k in range(4)]
    fs4 = {k: torch.cat([fs[k]] * 4) for k in R.SET_KEYS}
    _, logged = PR.oracle_fit(HP, P0, _tables(m), fs4, lambda e: [list(range(6 * s, 6 * s + 6)) for s in range(4)], lambda e, s, B: pairs[s][0],
                              lambda e, s: pairs[s][1], 12, 1e-3, freqs=m.time_embedding.freqs.cpu())
    first, last = logged[0][0], logged[-1][0]
    assert last < 0.7 * first and all(logged[-1][j] < logged[0][j] for j in range(1, 4))
    stats = pretrain.fit(m, data * 4, dict(lr=1e-3, epochs=12, batch_size=6, shuffle=False), seed=SEED, noise_fn=lambda e, s: pairs[s][1],
                         times_fn=lambda e, s, B: pairs[s][0], log=lambda *_: None)
    assert stats[-1]["train_loss"] < 0.5 * (first + last), (stats[-1]["train_loss"], first, last)


# ---- (9) the drop-in round trip ------------------------------------------------------------------------------------------------------

def test_pretrain_through_the_dropin_round_trips_through_load_model(tmp_path):
    from matinvent_amd.structure import write_extxyz
    _, data = _fit_set()
    train = write_extxyz(data, str(tmp_path / "train.extxyz"))
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        import main as dropin_main
        tiny = ["+model.hparams.decoder.hidden_dim=64", "+model.hparams.decoder.num_layers=2", "+model.hparams.decoder.num_freqs=8",
                "+model.hparams.beta_scheduler.timesteps=20", "+model.hparams.sigma_scheduler.timesteps=20", "model.head_scale=0.1"]
        run_ = dropin_main.main(["expname=pre", "pipeline=pretrain", f"pipeline.train_path={train}", f"pipeline.val_path={train}", "pipeline.save_freq=1",
                                 "pipeline.train_cfg.epochs=2", "pipeline.train_cfg.batch_size=4", "pipeline.train_cfg.lr=0.001", "device=cuda:0"] + tiny)
        run = tmp_path / "exp_res" / "pre"
        assert len(run_.history) == 2 and "val_loss" in run_.history[0]
        for name in ("epoch_0000", "epoch_0001", "final"):
            assert (run / "models" / name / "last.ckpt").exists() and (run / "models" / name / "hparams.yaml").exists()
        from matinvent_amd.suite import DiffCSPSuite
        s = DiffCSPSuite("diffcsp", {"batch_size": 3, "num_batches": 1}, {"batch_size": 2}, model_path=str(run / "models" / "final"), device="cuda:0")
        m2 = s.load_model()
        assert torch.equal(m2.decoder.theta.cpu(), run_.model.decoder.theta.detach().cpu())
        first = DiffCSPSuite("diffcsp", {"batch_size": 3, "num_batches": 1}, {"batch_size": 2}, model_path=str(run / "models" / "epoch_0000"),
                             device="cuda:0").load_model()
        assert not torch.equal(first.decoder.theta, m2.decoder.theta)
        assert m2.beta_scheduler.timesteps == 20
        final, _ = m2.sample(SimpleNamespace(num_atoms=torch.tensor([3, 5, 2])), seed=1)
        assert all(bool(torch.isfinite(final[k]).all()) for k in ("atom_types", "frac_coords", "lattices")) and final["frac_coords"].shape == (10, 3)
    finally:
        os.chdir(cwd)
        sys.path.remove(os.path.join(ROOT, "dropin"))


# ---- (10) memory ----------------------------------------------------------------------------------------------------------------------

def test_device_memory_does_not_grow_with_the_number_of_distinct_mini_batches():
    """5 mini-batches of distinct atom counts, then 30 more (none larger than the first): free device memory after the 30 must not lie
    below the value after the 5 by more than one mini-batch handle's footprint, measured here as the drop across creating one."""
    from matinvent_amd import pretrain
    from matinvent_amd.data import CrystalData
    m = make_module(64, 2, 8, T, _params(), sigmas_norm=_sigmas_norm())
    gen = torch.Generator().manual_seed(0)

    def batch(k):   # 8 crystals; the counts of no two k agree, and every count of k >= 1 is at most that of k = 0
        na = [20, 19, 18, 17, 16, 16, 5, 3] if k == 0 else [20, 19, 18, 17, 1 + k % 16, 1 + k // 16, 5, 3]
        return [CrystalData(torch.rand(n, 3, generator=gen), torch.randint(1, 95, (n,), generator=gen), 4 + 6 * torch.rand(1, 3, generator=gen),
                            70 + 40 * torch.rand(1, 3, generator=gen)) for n in na], na
    seen = set()

    def run(k):
        items, na = batch(k)
        assert tuple(na) not in seen
        seen.add(tuple(na))
        pretrain.train_step(m, pretrain._as_batch(items, m.device), pretrain.draw_times(len(na), T, 0, k, SEED), seed=SEED)
    for k in range(5):
        run(k)
    torch.cuda.synchronize()
    free_5 = torch.cuda.mem_get_info()[0]
    cb = m.make_batch(batch(0)[1])
    torch.cuda.synchronize()
    footprint = free_5 - torch.cuda.mem_get_info()[0]
    cb.release()
    assert footprint > 0
    for k in range(5, 35):
        run(k)
    torch.cuda.synchronize()
    free_35 = torch.cuda.mem_get_info()[0]
    assert free_5 - free_35 <= footprint, (free_5, free_35, footprint)
    assert len(m.__dict__.get("_nb_cache", {})) == 0   # (the module's handle cache was never touched)

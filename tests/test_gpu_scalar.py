"""GPU checks of the property predictor (matinvent_amd/csrc/scalar_head.hip under include/matinvent_hip_scalar.h; matinvent_amd.predictor;
rewards.Surrogate) against tests/scalar_ref.py.

Shapes: LOOP_NA = [1, 2, 171, 20, 3] (the one-atom mean, the longest crystal) and GRID_NA = [1, 3, 2] x 100 (300 crystals: several
blocks of every per-crystal and per-element launch); P = 1 and P = 3; hidden_dim 64 (the smallest the net accepts) and 512.
(1) The head with the trunk taken out: the device's own final node features (mi_cspnet_tap behind the final LayerNorm: tap index L + 1,
the rows the head pools) give mean, head, loss, statistics, seeds and the head's gradients in float64; the device within 4 x the float32
formulas' own deviation from float64, floor 4 * 2^-24 (tests/test_gpu_ft_arithmetic._check, DESIGN 25's rule).
(2) End to end on g15's weights and inputs against scalar_ref float32 at 2e-5 of max(1, |ref|) (tests/test_gpu_forward.py's bound for
lattice_out at that configuration); the inference and the taped form agree to the same; the `times` array and a non-zero `t_all` at the
same bound; predict on a collated batch and with a crystal its handle refuses.
(3) Gradients against scalar_ref float32 autograd at 2e-5 of max|ref| per tensor (tests/test_gpu_pretrain.py's bound); the three
diffusion heads' slices untouched; two micro-steps into one buffer.  (4) masks and shards  (5) no leak, pooled handles  (6) refusals
(7) fit_predictor on a toy set, the model directory, Surrogate through Reward.scoring."""
import ctypes as C
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import diffcsp_oracle as O
from tests import scalar_ref as SR
from tests.test_gpu_ft_arithmetic import _all
from tests.test_gpu_train import _rel

pytestmark = pytest.mark.gpu

L, F, TD = 2, 8, 256
LOOP_NA = [1, 2, 171, 20, 3]
GRID_NA = [1, 3, 2] * 100
HEAD_SLICES = ("lattice_out.weight", "type_out.weight", "type_out.bias", "coord_out.weight")


def test_the_shapes_reach_what_they_are_chosen_for():
    assert min(LOOP_NA) == 1 and max(LOOP_NA) == 171 and len(GRID_NA) == 300 and set(GRID_NA) == {1, 2, 3}
    assert 256 < len(GRID_NA) < 512 and len(GRID_NA) % 256 != 0 and sum(GRID_NA) * 64 > 4 * 256   # a second, partial trip of the stats loop; blocks of the per-element launches


@functools.lru_cache(maxsize=None)
def _model(H, P, seed=5):
    from matinvent_amd.predictor import PropertyPredictor
    m = PropertyPredictor([f"p{k}" for k in range(P)], hidden_dim=H, num_layers=L, time_dim=TD, num_freqs=F, ln=True, device="cuda", seed=seed)
    gen = torch.Generator().manual_seed(seed + 100)
    for k, w in m.trunk.views().items():   # perturbed LayerNorm parameters: their gradients are not those of the identity
        if "layer_norm" in k:
            w.add_((0.1 * torch.randn(w.shape, generator=gen)).cuda())
    m.mark_dirty()
    return m


def _P(m):
    return {"decoder." + k: v.detach().cpu() for k, v in m.state_dict().items()}


def _hp(H):
    return O.CSPNetHParams(hidden_dim=H, num_layers=L, num_freqs=F)


def _ns(fs):
    return SimpleNamespace(num_atoms=fs["num_atoms"], lengths=fs["lengths"], angles=fs["angles"], frac_coords=fs["frac"], atom_types=fs["atom_types"])


def _targets(B, P, seed, extra=(2, 0, 5)):
    g = torch.Generator().manual_seed(seed)
    yhat = torch.randn(B, P, generator=g)
    have = (torch.rand(B, P, generator=g) < 0.7).int()
    have[0] = 1
    have[1] = 0                      # a crystal whose targets are all missing
    yhat[have == 0] = float("nan")   # (the device never reads them)
    cg = have.sum(dim=0) + torch.tensor(extra[:P])
    return yhat.numpy(), have.numpy(), cg.numpy().astype(np.int32)


def _read(m, cb, P):
    from matinvent_amd import _lib
    from matinvent_amd.cspnet import _ptr, _stream
    gf = torch.empty(cb.num_graphs, m.hidden_dim, device="cuda")
    dout = torch.empty(cb.num_graphs, P, device="cuda")
    _lib.check(_lib.load().mi_scalar_read(cb._h, P, _ptr(gf), _ptr(dout), _stream()), "mi_scalar_read")
    return gf, dout


def _clean(fs, dtype=torch.float32):
    return SR.clean_inputs(fs["atom_types"], fs["frac"], fs["lengths"], fs["angles"], torch.zeros(len(fs["num_atoms"])), TD, dtype)


# ---- (1) the head with the trunk taken out --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,P,shape,kind", [(64, 1, "loop", "mse"), (64, 3, "grid", "l1"), (512, 3, "loop", "mse"), (512, 1, "grid", "l1"),
                                            (64, 3, "loop", "l1")])
def test_head_loss_seeds_and_statistics_vs_float64_of_the_devices_own_features(H, P, shape, kind):
    from matinvent_amd import predictor as PR
    m = _model(H, P)
    na = LOOP_NA if shape == "loop" else GRID_NA
    fs = SR.build_set(na, seed=31)
    B, ACC = len(na), 3
    yhat, have, cg = _targets(B, P, seed=7)
    cb = m.make_batch(na)
    grad, stats, out = torch.zeros_like(m.flat), torch.zeros(PR.stats_len(P), device="cuda"), torch.empty(B, P, device="cuda")
    PR.train_step(m, _ns(fs), yhat=yhat, have=have, grad=grad, stats=stats, count_global=cg, accum_steps=ACC, loss=kind, out=out, handle=cb)
    hf = m.trunk.tap(cb, L + 1).cpu()
    gf, dout = _read(m, cb, P)
    _, gW, gb = m.head_slices(grad)
    _, W, bias = (v.detach().cpu() for v in m.head_slices())
    ref = {}
    for dt in (torch.float64, torch.float32):
        g_ = SR.pooled(hf.to(dt), na)
        o_ = SR.head(g_, W.view(P, H).to(dt), bias.to(dt))
        d_ = SR.seeds(o_, yhat, have, cg, kind, ACC)
        ref[dt] = dict(gf=g_, out=o_, stats=SR.stats(o_, yhat, have, cg, kind), dout=d_, gb=d_.sum(dim=0), gW=d_.t() @ g_)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    what = f"H={H} P={P} {shape} {kind}"
    checks = [((gf, r64["gf"], r32["gf"], f"{what} gf"), {}), ((out, r64["out"], r32["out"], f"{what} out"), {}),
              ((dout, r64["dout"], r32["dout"], f"{what} d_out"), {}), ((gb, r64["gb"], r32["gb"], f"{what} grad_bias"), {}),
              ((gW.view(P, H), r64["gW"], r32["gW"], f"{what} grad_W"), {})]
    checks += [((stats[k:k + 1], r64["stats"][k:k + 1], r32["stats"][k:k + 1], f"{what} stats[{k}]"), {}) for k in range(PR.stats_len(P))]
    _all(checks)
    assert torch.count_nonzero(dout[torch.from_numpy(have == 0).cuda()]) == 0 and torch.isfinite(grad).all()
    assert stats[3::3].tolist() == have.sum(axis=0).tolist()
    # the inference form on the same handle: the head of ITS features, same bound; the forward-only form gives the same bits as the inference form
    o2 = PR.forward(m, _ns(fs), handle=cb)
    hf2 = m.trunk.tap(cb, L + 1).cpu()
    h64, h32 = (SR.head(SR.pooled(hf2.to(dt), na), W.view(P, H).to(dt), bias.to(dt)) for dt in (torch.float64, torch.float32))
    _all([((o2, h64, h32, f"{what} inference out"), {})])
    o3, s3 = torch.empty(B, P, device="cuda"), torch.zeros(PR.stats_len(P), device="cuda")
    PR.train_step(m, _ns(fs), yhat=yhat, have=have, stats=s3, count_global=cg, loss=kind, out=o3, handle=cb, forward_only=True)
    assert torch.equal(o3, o2)
    cb.release()


# ---- (2) end to end on the reference's fixture -------------------------------------------------------------------------------------------

def _close(a, b, tol, what):
    a, b = a.detach().cpu().double().numpy(), np.asarray(b, dtype=np.float64)
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    if os.environ.get("MI_TOL_REPORT"):
        print(f"TOL {what}: measured {err / scale:.3e}, demanded {tol:.0e}")
    assert err <= tol * scale, f"{what}: max abs err {err:.3e} > {tol:.1e} * {scale:.3g}"


def test_end_to_end_on_the_reference_fixture(golden):
    from matinvent_amd import predictor as PR
    from tests.gpu_util import params_from_golden
    g = golden("g15_pred_scalar")
    P = params_from_golden(g)
    m = PR.PropertyPredictor(["y"], hidden_dim=64, num_layers=2, time_dim=256, num_freqs=8, ln=True, device="cuda", seed=0)
    m.load_state_dict({k[len("decoder."):]: v for k, v in P.items()})
    assert list(m.state_dict())[:2] == ["scalar_out.weight", "scalar_out.bias"] and m.flat.numel() == m.n_trunk + 64 + 1
    fs = dict(num_atoms=torch.from_numpy(g["num_atoms"]), lengths=torch.from_numpy(g["lengths"]), angles=torch.from_numpy(g["angles"]),
              frac=torch.from_numpy(g["frac"]), atom_types=torch.from_numpy(g["atom_types"]))
    ref, _, _ = SR.forward(P, _hp(64), *_clean(fs), fs["num_atoms"])
    inf = PR.forward(m, _ns(fs))
    taped = torch.empty(3, 1, device="cuda")
    PR.train_step(m, _ns(fs), yhat=np.zeros((3, 1), np.float32), have=np.ones((3, 1), np.int32), grad=torch.zeros_like(m.flat), out=taped)
    _close(inf, ref, 2e-5, "inference form vs scalar_ref float32")
    _close(taped, ref, 2e-5, "taped form vs scalar_ref float32")
    _close(inf, g["scalar"], 2e-5, "inference form vs the reference's output")
    _close(inf, taped.cpu(), 2e-5, "inference form vs taped form")
    y = m.predict([SimpleNamespace(species=fs["atom_types"][1:8].tolist(), frac_coords=g["frac"][1:8], lengths=g["lengths"][1], angles=g["angles"][1])])
    assert y.shape == (1, 1) and abs(y[0, 0] - float(inf[1, 0])) <= 2e-5 * max(1.0, abs(float(inf[1, 0])))


def _g15(golden):
    from matinvent_amd import predictor as PR
    from tests.gpu_util import params_from_golden
    g = golden("g15_pred_scalar")
    P = params_from_golden(g)
    m = PR.PropertyPredictor(["y"], hidden_dim=64, num_layers=2, time_dim=256, num_freqs=8, ln=True, device="cuda", seed=0)
    m.load_state_dict({k[len("decoder."):]: v for k, v in P.items()})
    fs = dict(num_atoms=torch.from_numpy(g["num_atoms"]), lengths=torch.from_numpy(g["lengths"]), angles=torch.from_numpy(g["angles"]),
              frac=torch.from_numpy(g["frac"]), atom_types=torch.from_numpy(g["atom_types"]))
    return m, P, fs


def test_the_time_embedding_at_non_zero_times(golden):
    """The `times` array and a non-zero `t_all` of both entries (kept in the ABI for a time-dependent predictor; the predictor itself
    runs at time 0, where sin and cos hide the index and the frequency of every column): g15's weights and crystals at the times
    [3, 0, 17] and at t_all = 5 against scalar_ref float32 at the end-to-end bound, 2e-5 of max(1, |ref|).  On these weights the
    reference's own outputs move by 0.4 to 1.0 between time 0 and these times."""
    from matinvent_amd import predictor as PR
    m, P, fs = _g15(golden)
    ins = lambda times: SR.clean_inputs(fs["atom_types"], fs["frac"], fs["lengths"], fs["angles"], torch.tensor(times), TD, torch.float32)
    ref0, reft, ref5 = (SR.forward(P, _hp(64), *ins(t), fs["num_atoms"])[0] for t in ([0, 0, 0], [3, 0, 17], [5, 5, 5]))
    assert float((reft - ref0).abs()[[0, 2]].min()) > 0.1 and float((ref5 - ref0).abs().min()) > 0.1 and float((reft - ref0).abs()[1]) == 0.0
    _close(PR.forward(m, _ns(fs), times=[3, 0, 17]), reft, 2e-5, "inference form at times [3, 0, 17]")
    o5 = PR.forward(m, _ns(fs), t_all=5)
    _close(o5, ref5, 2e-5, "inference form at t_all = 5")
    assert torch.equal(PR.forward(m, _ns(fs), times=[5, 5, 5]), o5)
    kw = dict(yhat=np.zeros((3, 1), np.float32), have=np.ones((3, 1), np.int32))
    for what, tkw, ref in (("times [3, 0, 17]", dict(times=[3, 0, 17]), reft), ("t_all = 5", dict(t_all=5), ref5)):
        taped, fo = torch.empty(3, 1, device="cuda"), torch.empty(3, 1, device="cuda")
        PR.train_step(m, _ns(fs), grad=torch.zeros_like(m.flat), out=taped, **kw, **tkw)
        PR.train_step(m, _ns(fs), forward_only=True, out=fo, **kw, **tkw)
        _close(taped, ref, 2e-5, f"taped form at {what}")
        _close(fo, ref, 2e-5, f"forward-only form at {what}")


def test_predict_takes_a_collated_batch_and_gives_nan_for_a_crystal_the_handle_refuses():
    """predict on a CrystalBatchData equals predict on its records; on a knn predictor (whose batch handle takes at most 64 atoms per
    crystal) a 70-atom crystal inside a mini-batch makes the handle of that mini-batch refuse: the others are evaluated one by one and
    equal what they are without it, the refused crystal is a row of NaN."""
    from matinvent_amd import _lib
    from matinvent_amd import predictor as PR
    from matinvent_amd.data import CrystalBatchData, CrystalData
    m = _model(64, 3)
    fs = SR.build_set([1, 7, 20, 3, 13], seed=35)
    off = np.concatenate([[0], np.cumsum(fs["num_atoms"].numpy())])
    recs = [CrystalData(fs["frac"][off[i]:off[i + 1]], fs["atom_types"][off[i]:off[i + 1]], fs["lengths"][i:i + 1], fs["angles"][i:i + 1])
            for i in range(5)]
    y = m.predict(recs, batch_size=2)
    assert y.shape == (5, 3) and np.isfinite(y).all()
    assert np.array_equal(m.predict(CrystalBatchData(recs), batch_size=2), y)
    assert np.array_equal(m.predict(CrystalBatchData(recs).to("cuda"), batch_size=2), y)
    k = PR.PropertyPredictor(["a", "b"], hidden_dim=64, num_layers=L, time_dim=TD, num_freqs=F, ln=True, edge_style="knn", device="cuda", seed=9)
    with pytest.raises(_lib.MIError, match="exceeds the supported 64"):
        k.make_batch([3, 70])
    fk = SR.build_set([3, 5, 70, 4], seed=39)
    ok_ = np.concatenate([[0], np.cumsum(fk["num_atoms"].numpy())])
    rk = [CrystalData(fk["frac"][ok_[i]:ok_[i + 1]], fk["atom_types"][ok_[i]:ok_[i + 1]], fk["lengths"][i:i + 1], fk["angles"][i:i + 1]) for i in range(4)]
    small = [rk[0], rk[1], rk[3]]
    alone = np.concatenate([k.predict([r]) for r in small])
    assert np.isfinite(alone).all()
    yk = k.predict(rk, batch_size=3)            # mini-batches [3, 5, 70] (refused, retried one by one) and [4]
    assert np.isnan(yk[2]).all() and np.array_equal(yk[[0, 1, 3]], alone)
    assert np.array_equal(k.predict(CrystalBatchData(rk), batch_size=8)[[0, 1, 3]], alone) and np.isnan(k.predict([rk[2]])).all()


# ---- (3) gradients ------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _grad_case(H, P, kind):
    m = _model(H, P)
    fs = SR.build_set(LOOP_NA, seed=33)
    c = SimpleNamespace(m=m, fs=fs, B=len(LOOP_NA), ACC=2, kind=kind, tg=[_targets(len(LOOP_NA), P, seed=11 + k) for k in range(2)])
    Pd = _P(m)
    c.ref = [SR.micro_step(Pd, _hp(H), *_clean(fs), fs["num_atoms"], *tg, kind=kind, accum=c.ACC) for tg in c.tg]   # computed once, left unchanged
    return c


def _dev_grads(m, flat):
    t, gW, gb = m.head_slices(flat)
    out = {"decoder." + k: t[o:o + n].view(shape) for k, (o, n, shape) in m.trunk.layout.items()}
    out["decoder.scalar_out.weight"], out["decoder.scalar_out.bias"] = gW.view(m.P, m.hidden_dim), gb
    return out


def _grads_close(m, flat, ref, what, tol=2e-5):
    for k, g in _dev_grads(m, flat).items():
        if k[len("decoder."):] in HEAD_SLICES:
            assert torch.count_nonzero(g) == 0 and torch.count_nonzero(ref[k]) == 0, k
        else:
            _rel(g, ref[k].numpy(), tol, f"{what}: grad {k}")


@pytest.mark.parametrize("H,P,kind", [(64, 3, "mse"), (64, 1, "l1"), (512, 3, "mse")])
def test_gradients_vs_scalar_ref_autograd(H, P, kind):
    """Every trunk tensor, grad_W and grad_bias within 2e-5 of max|ref| of float32 autograd (measured, MI_TOL_REPORT=1: see DESIGN 42);
    a second micro-step with other targets into the same buffers gives the sum of the references; with the gradient prefilled with a
    non-zero pattern the lattice_out.*, type_out.* and coord_out.* slices are the pattern afterwards, bit for bit."""
    from matinvent_amd import predictor as PR
    c = _grad_case(H, P, kind)
    m = c.m
    grad, stats = torch.zeros_like(m.flat), torch.zeros(PR.stats_len(P), device="cuda")
    kw = dict(accum_steps=c.ACC, loss=kind)
    PR.train_step(m, _ns(c.fs), yhat=c.tg[0][0], have=c.tg[0][1], count_global=c.tg[0][2], grad=grad, stats=stats, **kw)
    _grads_close(m, grad, c.ref[0]["grads"], f"H={H} P={P} {kind}")
    _rel(stats, c.ref[0]["stats"].numpy(), 1e-4, "statistics")
    PR.train_step(m, _ns(c.fs), yhat=c.tg[1][0], have=c.tg[1][1], count_global=c.tg[1][2], grad=grad, stats=stats, **kw)
    both = {k: c.ref[0]["grads"][k] + c.ref[1]["grads"][k] for k in c.ref[0]["grads"]}
    _grads_close(m, grad, both, f"H={H} P={P} {kind}, two micro-steps")
    _rel(stats, (c.ref[0]["stats"] + c.ref[1]["stats"]).numpy(), 1e-4, "statistics of two micro-steps")
    pattern = torch.full_like(m.flat, 0.375)
    g2 = pattern.clone()
    PR.train_step(m, _ns(c.fs), yhat=c.tg[0][0], have=c.tg[0][1], count_global=c.tg[0][2], grad=g2, **kw)
    for k, g in _dev_grads(m, g2).items():
        if k[len("decoder."):] in HEAD_SLICES:
            assert torch.equal(g, torch.full_like(g, 0.375)), k
        else:
            assert not torch.equal(g, torch.full_like(g, 0.375)), k


# ---- (4) masks and shards -----------------------------------------------------------------------------------------------------------------

def test_a_crystal_without_targets_changes_no_gradient_bit():
    from matinvent_amd import predictor as PR
    m = _model(64, 3)
    fs = SR.build_set([1, 7, 20, 3, 13], seed=35)
    yhat, have, cg = _targets(5, 3, seed=13)
    assert have[1].sum() == 0
    res = []
    for fill in (float("nan"), 4.5):
        y = yhat.copy()
        y[1] = fill
        grad, stats = torch.zeros_like(m.flat), torch.zeros(PR.stats_len(3), device="cuda")
        PR.train_step(m, _ns(fs), yhat=y, have=have, count_global=cg, grad=grad, stats=stats)
        res.append((grad, stats))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert torch.isfinite(res[0][0]).all() and float(res[0][0].abs().max()) > 0


@pytest.mark.parametrize("kind", ["mse", "l1"])
def test_two_shards_sum_to_the_unsplit_batch(kind):
    """[1, 7] and [20, 3, 13] as two handles with their node / graph offsets and the whole batch's count_global against the unsplit call."""
    from matinvent_amd import predictor as PR
    m = _model(64, 3)
    na = [1, 7, 20, 3, 13]
    fs = SR.build_set(na, seed=35)
    yhat, have, _ = _targets(5, 3, seed=13)
    cg = have.sum(axis=0).astype(np.int32)
    g0, s0 = torch.zeros_like(m.flat), torch.zeros(PR.stats_len(3), device="cuda")
    PR.train_step(m, _ns(fs), yhat=yhat, have=have, count_global=cg, grad=g0, stats=s0, loss=kind)
    g1, s1 = torch.zeros_like(m.flat), torch.zeros(PR.stats_len(3), device="cuda")
    for idx, off in (([0, 1], (0, 0)), ([2, 3, 4], (8, 2))):
        PR.train_step(m, _ns(SR.subset(fs, idx)), yhat=yhat[idx], have=have[idx], count_global=cg, grad=g1, stats=s1, loss=kind, offsets=off)
    ref = _dev_grads(m, g0)
    for k, g in _dev_grads(m, g1).items():
        if k[len("decoder."):] not in HEAD_SLICES:
            _rel(g, ref[k].cpu().numpy(), 2e-5, f"shards {kind}: grad {k}")
    _rel(s1, s0.cpu().numpy(), 1e-5, "shards: statistics")


# ---- (5) no leak ----------------------------------------------------------------------------------------------------------------------------

def test_predictor_calls_leave_nothing_on_the_handle_and_pooled_handles_give_the_same_bits():
    from matinvent_amd import predictor as PR
    from matinvent_amd.pool import HandlePool
    m = _model(64, 3)
    na = [1, 7, 20, 3, 13]
    fs = SR.build_set(na, seed=35)
    yhat, have, cg = _targets(5, 3, seed=13)
    t_emb, onehot, fr, lat = (v.cuda() for v in _clean(fs))
    cb = m.make_batch(na)
    before = m.trunk(t_emb, onehot, fr, lat, None, batch=cb)
    o_classic = PR.forward(m, _ns(fs), handle=cb)
    g_classic, s_classic = torch.zeros_like(m.flat), torch.zeros(PR.stats_len(3), device="cuda")
    PR.train_step(m, _ns(fs), yhat=yhat, have=have, count_global=cg, grad=g_classic, stats=s_classic, handle=cb)
    PR.train_step(m, _ns(fs), yhat=yhat, have=have, count_global=cg, stats=torch.zeros_like(s_classic), handle=cb, forward_only=True)
    after = m.trunk(t_emb, onehot, fr, lat, None, batch=cb)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    cb.release()
    pool = HandlePool(poison=True)
    try:
        for _ in range(2):   # (the second round runs on recycled, poisoned blocks)
            o_pool = PR.forward(m, _ns(fs), pool=pool)
            g_pool, s_pool = torch.zeros_like(m.flat), torch.zeros(PR.stats_len(3), device="cuda")
            PR.train_step(m, _ns(fs), yhat=yhat, have=have, count_global=cg, grad=g_pool, stats=s_pool, pool=pool)
            assert torch.equal(o_pool, o_classic) and torch.equal(g_pool, g_classic) and torch.equal(s_pool, s_classic)
        torch.cuda.synchronize()
    finally:
        pool.close()


# ---- (6) refusals of the C entries ----------------------------------------------------------------------------------------------------------

def test_refusals_before_anything_is_enqueued():
    from matinvent_amd import _lib, guidance
    from matinvent_amd import predictor as PR
    from matinvent_amd.conditioning import Condition
    from matinvent_amd.cspnet import CSPNet, _ptr, _stream
    lib = _lib.load()
    m = _model(64, 3)
    na = [2, 3]
    fs = SR.build_set(na, seed=37)
    b = _ns(fs)
    f = lambda x: x.cuda().float().contiguous()
    lengths, angles, frac, at = f(b.lengths), f(b.angles), f(b.frac_coords), b.atom_types.cuda().int().contiguous()
    yh, hv = np.zeros((2, 3), np.float32), np.ones((2, 3), np.int32)
    yd, hd = torch.from_numpy(yh).cuda(), torch.from_numpy(hv).cuda()
    m.trunk.sync()
    _, W, bias = m.head_slices()
    grad, stats, out = torch.zeros_like(m.flat), torch.zeros(PR.stats_len(3), device="cuda"), torch.full((2, 3), 7.0, device="cuda")
    gt, gW, gb = m.head_slices(grad)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))

    def step(net, cb, P=3, yhat=yd, have=hd, have_h=hv, cg=(2, 2, 2), accum=1, kind=0, train=True):
        cgh = np.asarray(cg, np.int32)
        cgd = torch.from_numpy(cgh).cuda()
        rc = lib.mi_scalar_micro_step(net._h, cb._h, _ptr(lengths), _ptr(angles), _ptr(frac), _ptr(at), _ptr(m.time_freqs), None, 0, _ptr(W), _ptr(bias),
                                      P, _ptr(yhat), _ptr(have), None if have_h is None else ip(have_h), _ptr(cgd), ip(cgh), accum, kind,
                                      _ptr(gt) if train else None, _ptr(gW) if train else None, _ptr(gb) if train else None, _ptr(stats), _ptr(out),
                                      _stream())
        return rc, lib.mi_last_error().decode()

    def fwd(net, cb):
        rc = lib.mi_scalar_forward(net._h, cb._h, _ptr(lengths), _ptr(angles), _ptr(frac), _ptr(at), _ptr(m.time_freqs), None, 0, _ptr(W), _ptr(bias), 3,
                                   _ptr(out), _stream())
        return rc, lib.mi_last_error().decode()

    def refused(rc_msg, text):
        rc, msg = rc_msg
        assert rc == _lib.MI_EINVAL and text in msg, (rc, msg)

    cb = m.make_batch(na)
    refused(step(m.trunk, cb, P=0), "at least 1")
    refused(step(m.trunk, cb, have=None, have_h=None), "yhat without have")
    refused(step(m.trunk, cb, cg=(2, 1, 2)), "count_global[1] = 1 is below the handle's 2 present targets")
    refused(step(m.trunk, cb, accum=0), "accum_steps")
    refused(step(m.trunk, cb, kind=2), "loss_kind")
    tm = np.array([0, 1, 2], np.int32)
    _lib.check(lib.mi_batch_set_time_map(cb._h, ip(tm), 3))
    refused(step(m.trunk, cb), "time map")
    refused(fwd(m.trunk, cb), "time map")
    _lib.check(lib.mi_batch_set_time_map(cb._h, None, 0))
    zn, zb = np.zeros(5, np.int32), np.zeros(2, np.int32)
    _lib.check(lib.mi_batch_set_likelihood_mask(cb._h, ip(zn), ip(zn), ip(zb)))
    refused(step(m.trunk, cb), "a condition or a likelihood mask")
    refused(fwd(m.trunk, cb), "a condition or a likelihood mask")
    _lib.check(lib.mi_batch_set_likelihood_mask(cb._h, None, None, None))
    # a replacement condition, alone (the likelihood mask is cleared): every atom type known
    cond = Condition.composition([{"Na": 2}, {"Si": 3}], 2)
    cond.attach(None, cb, table=torch.ones(3, 3))
    refused(step(m.trunk, cb), "a condition or a likelihood mask")
    refused(step(m.trunk, cb, train=False), "a condition or a likelihood mask")
    refused(fwd(m.trunk, cb), "a condition or a likelihood mask")
    Condition.clear(cb)
    # guidance: gamma = 0 takes no partner and asks nothing of the net
    guidance.attach(cb, None, yh, hv, 2, 0.0)
    refused(step(m.trunk, cb), "carries guidance")
    refused(step(m.trunk, cb, train=False), "carries guidance")
    refused(fwd(m.trunk, cb), "carries guidance")
    guidance.clear(cb)
    assert step(m.trunk, cb, train=False)[0] == 0 and fwd(m.trunk, cb)[0] == 0   # ... and with each of them cleared the handle is taken again
    # an open weight-gradient window, empty: the taped form alone is refused
    cb.set_wgrad_window(m.trunk, 2)
    refused(step(m.trunk, cb), "open weight-gradient window")
    assert step(m.trunk, cb, train=False)[0] == 0   # (the forward-only form runs under an open window, as mi_pretrain_micro_step's does)
    # ... and with one micro-step's weight gradients pending in it (a taped forward and backward of the trunk, not flushed): every form
    g_ = torch.Generator().manual_seed(41)
    temb, types = torch.randn(2, TD, generator=g_).cuda(), torch.randn(5, 100, generator=g_).cuda()
    lat = (torch.eye(3) * 5 + 0.1 * torch.randn(2, 3, 3, generator=g_)).cuda().contiguous()
    pl, px, pt = torch.empty(2, 3, 3, device="cuda"), torch.empty(5, 3, device="cuda"), torch.empty(5, 100, device="cuda")
    _lib.check(lib.mi_cspnet_forward_train(m.trunk._h, cb._h, _ptr(temb), _ptr(types), _ptr(frac), _ptr(lat), _ptr(pl), _ptr(px), _ptr(pt), _stream()))
    dl, dx, dt = torch.randn(2, 3, 3, generator=g_).cuda(), torch.randn(5, 3, generator=g_).cuda(), torch.randn(5, 100, generator=g_).cuda()
    g_trunk = torch.zeros_like(m.trunk.theta)
    _lib.check(lib.mi_cspnet_backward(m.trunk._h, cb._h, _ptr(dl), _ptr(dx), _ptr(dt), _ptr(g_trunk), _stream()))
    assert lib.mi_batch_wgrad_pending(cb._h) == 1
    refused(step(m.trunk, cb), "pending deferred weight gradients")
    refused(step(m.trunk, cb, train=False), "pending deferred weight gradients")
    refused(fwd(m.trunk, cb), "pending deferred weight gradients")
    assert lib.mi_batch_wgrad_pending(cb._h) == 1
    cb.wgrad_flush(m.trunk, g_trunk)
    cb.set_wgrad_window(m.trunk, 0)
    assert step(m.trunk, cb, train=False)[0] == 0
    # mi_scalar_read takes the last call's P alone (d_out is laid out for it)
    gf_ = torch.empty(2, 64, device="cuda")
    assert lib.mi_scalar_read(cb._h, 3, _ptr(gf_), None, _stream()) == 0
    for bad in (2, 1, 4, 0):
        assert lib.mi_scalar_read(cb._h, bad, _ptr(gf_), None, _stream()) == _lib.MI_ESTATE and b"properties" in lib.mi_last_error()
    cb.release()
    fresh = m.make_batch(na)
    assert lib.mi_scalar_read(fresh._h, 3, _ptr(gf_), None, _stream()) == _lib.MI_ESTATE
    fresh.release()
    latent = CSPNet(hidden_dim=64, num_layers=L, num_freqs=F, latent_dim=TD + 16, ln=True, smooth=True, pred_type=True, device="cuda")
    _lib.check(lib.mi_net_set_latent(latent._h, 1, 8))
    assert lib.mi_net_latent_dim(latent._h) > 0
    latent.sync()
    cl = latent.make_batch(na)
    refused(step(latent, cl), "property-conditioned embedding")
    refused(fwd(latent, cl), "property-conditioned embedding")
    cl.release()
    for name in ("mi_scalar_forward", "mi_scalar_micro_step"):   # the net first, nothing else: the refusal is the entry's first line, as its siblings'
        args = [latent._h if k == 0 else 0 if ty is C.c_int else None for k, ty in enumerate(_lib.SCALAR_SIGNATURES[name][1])]
        assert getattr(lib, name)(*args) == _lib.MI_EINVAL, name
        assert b"mi_net_set_latent" in lib.mi_last_error() and name.encode() in lib.mi_last_error(), name
    torch.cuda.synchronize()
    assert torch.count_nonzero(grad) == 0   # (no refused call reached the gradient; the forward-only calls that ran take none)
    e = m.make_batch([])   # B = 0: MI_OK, nothing launched
    rc = lib.mi_scalar_micro_step(m.trunk._h, e._h, None, None, None, None, None, None, 0, None, None, 3, None, None, None, None, None, 1, 0,
                                  None, None, None, None, None, _stream())
    assert rc == 0
    e.release()


# ---- (7) fit_predictor, the model directory, Surrogate --------------------------------------------------------------------------------------

def _toy(n, seed):
    """Random crystals of 2-8 atoms whose property is the mean atomic number: linear in the pooled one-hot input."""
    from matinvent_amd.data import CrystalData
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        k = int(torch.randint(2, 9, (1,), generator=g))
        z = torch.randint(1, 60, (k,), generator=g)
        out.append(CrystalData(torch.rand(k, 3, generator=g), z, 4.0 + 4.0 * torch.rand(1, 3, generator=g), 80.0 + 20.0 * torch.rand(1, 3, generator=g),
                               properties={"zbar": float(z.float().mean())}))
    return out


def test_fit_predictor_on_a_toy_set_and_the_model_directory(tmp_path):
    from matinvent_amd import predictor as PR
    from matinvent_amd.rewards import Reward, Surrogate
    from tests.gpu_util import make_module
    train, val = _toy(40, seed=1), _toy(12, seed=2)
    cfg = dict(lr=3e-3, epochs=6, batch_size=16, max_grad_norm=10.0, skip_nonfinite_steps=True, handle_pool=True)
    runs = []
    for _ in range(2):
        m = PR.PropertyPredictor(["zbar"], hidden_dim=64, num_layers=2, time_dim=256, num_freqs=8, ln=True, device="cuda", seed=3)
        hist = PR.fit_predictor(m, train, cfg, val_list=val, seed=4, log=lambda s: None)
        runs.append((m, hist))
    (m, hist), (m2, hist2) = runs
    assert torch.equal(m.flat.data, m2.flat.data) and hist == hist2
    assert len(hist) == 6 and hist[-1]["train_loss"] < hist[0]["train_loss"]
    assert all(np.isfinite(d["val_loss"]) and np.isfinite(d["val_mse_zbar"]) for d in hist)
    ev = PR.evaluate(m, val, batch_size=5)["zbar"]
    ev1 = PR.evaluate(m, val, batch_size=12)["zbar"]
    assert ev["count"] == 12 and abs(ev["mse"] - ev1["mse"]) <= 1e-5 * ev1["mse"] and abs(ev["mae_raw"] - ev1["mae_raw"]) <= 1e-5 * ev1["mae_raw"]
    assert abs(ev1["mse"] - hist[-1]["val_mse_zbar"]) <= 1e-5 * ev1["mse"]
    yv = m.normalizer.raw(val)[:, 0]
    print(f"TOY validation mse (raw units) {ev1['mse_raw']:.4g} beside the variance of the validation targets {float(np.var(yv)):.4g}; "
          f"train_loss {hist[0]['train_loss']:.4g} -> {hist[-1]['train_loss']:.4g}")
    d = PR.save_predictor(m, str(tmp_path / "model"))
    m3 = PR.load_predictor(d, device="cuda", names=["zbar"])
    assert list(torch.load(os.path.join(d, "last.ckpt"), weights_only=False)["state_dict"])[:2] == ["scalar_out.weight", "scalar_out.bias"]
    y, y3 = m.predict(val, batch_size=5), m3.predict(val, batch_size=5)
    assert y.shape == (12, 1) and np.isfinite(y).all() and np.array_equal(y, y3)
    # a record the network cannot take is NaN, the others are what they were
    from matinvent_amd.data import SimpleStructure
    bad = SimpleStructure([4.0, 4.0, 4.0], [90.0, 90.0, 90.0], [0, 101], np.zeros((2, 3)))
    yb = m.predict([val[0], bad, val[1]], batch_size=8)
    assert np.isnan(yb[1]).all() and np.array_equal(yb[[0, 2]], m.predict(val[:2], batch_size=8))
    # the saved directory as a reward over sampled crystals
    mod = make_module(64, 2, 8, 20)
    from matinvent_amd.data import data2struc
    samples = _sampled(mod)
    strucs = [data2struc(s) for s in samples]
    rw = Reward(str(tmp_path / "rw"), [dict(name="zbar", calculator=Surrogate(model_path=d, task="zbar", device="cuda"), target="ascending",
                                             minv=0.0, maxv=60.0)], 0.5)
    r, props, failed = rw.scoring((strucs, None), "x")
    assert len(r) == len(strucs) and np.isfinite(r).all() and not failed.any() and np.isfinite(props["zbar"]).all()


def _sampled(mod):
    """A few crystals from a tiny DiffCSPModule.sample."""
    from matinvent_amd.data import CrystalData
    from matinvent_amd.data import lattices_to_params_shape
    from tests.gpu_util import Box
    na = [3, 5, 2, 4]
    traj = mod.sample(Box(na), step_lr=1e-5)
    last = traj[0] if isinstance(traj, tuple) else traj
    types, frac, lat = last["atom_types"], last["frac_coords"], last["lattices"]
    if types.dim() == 2:
        types = types.argmax(dim=-1) + 1
    lengths, angles = lattices_to_params_shape(lat.cpu())
    off = np.concatenate([[0], np.cumsum(na)])
    return [CrystalData(frac[off[i]:off[i + 1]].cpu(), types[off[i]:off[i + 1]].cpu().long(), lengths[i:i + 1], angles[i:i + 1]) for i in range(len(na))]

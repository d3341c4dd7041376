"""GPU checks of the property-conditioned prior and classifier-free guidance (matinvent_amd/csrc/guidance.hip; matinvent_amd.guidance;
DESIGN 41) against tests/guidance_ref.py and the oracle.

(1) the embedding rows against float64, (2) the combination against float64 -- both under DESIGN 25's rule as
tests/test_gpu_ft_arithmetic._check implements it (4 x the float32 CPU formula's own deviation from float64, floor 4 * 2^-24);
(3) the conditional micro-step against float32 oracle autograd at test_gpu_pretrain's bounds (2e-5 of max|ref| per gradient tensor, 1e-4
relative per statistic); (4) the guided chain against the reference chain at test_philox_chain_vs_oracle_and_sharding's set-up and bound
(3e-4, times 1 + 2 gamma with guidance); (5) exact identities; (6) the library's refusals; (7) fit -> evaluate -> save -> load."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tests.test_gpu_traj_arithmetic as TA
from oracle import diffcsp_oracle as O
from tests import ft_ref64 as R
from tests import guidance_ref as GR
from tests import pretrain_ref64 as PR
from tests.gpu_util import Box, load_decoder, make_module, wrap_dist
from tests.test_gpu_ft_arithmetic import _all, _tables
from tests.test_gpu_pretrain import NA_B, _grads_close, _ns, _sigmas_norm, _stats_close

pytestmark = pytest.mark.gpu

T = 1000
SEED = 1234
CALL = 17     # guidance.drop_mask(1234, 17, 5, 0.5) = [1 0 1 1 0]: dropped and kept crystals in both shards of [0:2] / [2:5]
F = 8
LOOP_NA = [1, 2, 85, 86, 3, 171]
YS = [0.0, 0.37, -0.37, 8.0, -8.0, 11.5]


def _names(P_):
    return ["density", "gap", "bulk"][:P_]


def _hp(P_, H=64):
    return O.CSPNetHParams(hidden_dim=H, num_layers=2, num_freqs=8, latent_dim=2 * F * P_)


def _module(P_, T_=T, P=None, sigmas_norm=None):
    m = make_module(64, 2, 8, T_, None, sigmas_norm=sigmas_norm, latent_dim=2 * F * P_, condition=dict(properties=_names(P_), num_freqs=F))
    if P is not None:
        load_decoder(m.decoder, P)
    return m


# ---- (1) the embedding ------------------------------------------------------------------------------------------------------------------

def _embedding_inputs(B, P_, top):
    g = np.random.default_rng(B + P_)
    times = g.integers(1, top + 1, size=B).astype(np.int32)
    times[0] = 1
    times[-1] = top
    if B > 2:
        times[1] = top
    y = np.array([YS[(i + 2 * p) % len(YS)] for i in range(B) for p in range(P_)], dtype=np.float64).reshape(B, P_)
    miss = g.random((B, P_)) < 0.25
    if B > 1:
        miss[0, 0], miss[1, 0] = False, True
    y[miss] = np.nan
    drop = g.random(B) < 0.3
    if B > 2:
        drop[2], drop[0] = True, False
    return times, y, drop


@pytest.mark.parametrize("mapped", [False, True], ids=["trained-grid", "time-map"])
@pytest.mark.parametrize("B", [1, 6, 300])
@pytest.mark.parametrize("P_", [1, 3])
def test_embedding_rows_vs_float64(P_, B, mapped):
    m0 = _module(P_)
    m = m0.respaced(4) if mapped else m0
    top = 4 if mapped else T
    times, y, drop = _embedding_inputs(B, P_, top)
    assert B != 300 or (B * (256 + 2 * F * P_)) % 256 != 0   # (300 rows: a partial last block)
    out = m.crystal_embedding(times, y, drop)
    tau = None if not mapped else m.time_map.numpy()
    tt = times if tau is None else tau[times]
    # the time columns: the bits of mi_time_embedding at the (mapped) times
    assert torch.equal(out[:, :256], m0.time_embedding(torch.from_numpy(tt)))
    yhat, have = np.nan_to_num(y).astype(np.float32), np.isfinite(y).astype(np.int32)
    freqs = m0.time_embedding.freqs.cpu()
    r64 = GR.embedding_row(times, freqs, yhat, have, drop, F, torch.float64, time_map=tau)
    r32 = GR.embedding_row(times, freqs, yhat, have, drop, F, torch.float32, time_map=tau)
    lat = out[:, 256:].cpu().reshape(B, P_, 2 * F)
    off = (have == 0) | drop[:, None]
    assert off.any() or B == 1
    assert torch.count_nonzero(lat[torch.from_numpy(off)]) == 0                    # the null columns: exactly 0
    on = lat[torch.from_numpy(~off)]
    if on.numel():
        assert float(((on[:, :F] ** 2 + on[:, F:] ** 2) - 1).abs().max()) < 1e-5   # ... which no value can be taken for
    _all([((out[:, 256:], r64[:, 256:], r32[:, 256:], f"latent columns P={P_} B={B} mapped={mapped}"), {})])
    # the null row of every crystal
    null = m.crystal_embedding(times)
    assert torch.equal(null[:, :256], out[:, :256]) and torch.count_nonzero(null[:, 256:]) == 0


# ---- (2) the combination ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gamma", [0.5, 2.0])
def test_combine_vs_float64(gamma):
    from matinvent_amd import _lib
    from matinvent_amd.cspnet import _ptr, _stream
    lib = _lib.load()
    B, N = len(LOOP_NA), sum(LOOP_NA)
    nl, nx, nt = B * 9, N * 3, N * 100   # the step's three arrays as the three segments of one: 54 lattice elements, then 1044, then 34800
    n = nl + nx + nt
    assert nl % 256 != 0 and (nl + nx) % 256 != 0 and n % 256 != 0   # (both segment boundaries and the end fall inside a block)
    g = torch.Generator().manual_seed(7)
    pc, pu = torch.randn(n, generator=g), torch.randn(n, generator=g)
    pu[::7] = pc[::7]
    dc, du, out = pc.cuda(), pu.cuda(), torch.empty(n, device="cuda")
    _lib.check(lib.mi_guidance_combine(_ptr(dc), _ptr(du), gamma, nl, nx, nt, _ptr(out), _stream()))
    _all([((out, GR.combine(pc, pu, gamma, torch.float64), GR.combine(pc, pu, gamma, torch.float32), f"combine gamma={gamma}"), {})])
    assert torch.equal(out.cpu()[::7], pc[::7])
    _lib.check(lib.mi_guidance_combine(_ptr(dc), _ptr(dc), gamma, nl, nx, nt, _ptr(out), _stream()))
    assert torch.equal(out, dc)                                                    # p_c == p_u gives exactly p_c
    # each segment alone, and in place: the same bits as its part of the whole
    for seg in ((n, 0, 0), (0, n, 0), (0, 0, n)):
        inplace = dc.clone()
        _lib.check(lib.mi_guidance_combine(_ptr(inplace), _ptr(du), gamma, *seg, _ptr(inplace), _stream()))
        _lib.check(lib.mi_guidance_combine(_ptr(dc), _ptr(du), gamma, nl, nx, nt, _ptr(out), _stream()))
        assert torch.equal(inplace, out)


@pytest.mark.parametrize("B,offset", [(300, 0), (300, 1237), (5, 2), (7, 2 ** 33 + 3)])
def test_device_drop_mask_is_the_host_contract(B, offset):
    """cond_drop_kernel behind mi_guidance_drop_mask -- what the conditional micro-step draws -- against guidance.drop_mask: 300 crystals (a
    partial second block), graph offsets that are no multiple of 4 (the Philox word inside a block) and beyond 2^32."""
    from matinvent_amd import _lib, guidance
    from matinvent_amd.cspnet import _ptr, _stream
    lib = _lib.load()
    for p in (0.5, 0.1, 1.0):
        out = torch.full((B + 1,), -7, dtype=torch.int32, device="cuda")
        _lib.check(lib.mi_guidance_drop_mask(SEED, CALL, offset, B, p, _ptr(out), _stream()))
        want = guidance.drop_mask(SEED, CALL, B, p, offset)
        assert out[:B].cpu().numpy().astype(bool).tolist() == want.tolist() and int(out[B]) == -7 and set(out[:B].tolist()) <= {0, 1}
        assert np.array_equal(want, GR.drop_mask(SEED, CALL, B, p, offset))
    assert B < 300 or 100 < int(guidance.drop_mask(SEED, CALL, B, 0.5, offset).sum()) < 200


# ---- (3) the conditional micro-step -------------------------------------------------------------------------------------------------------

def _params(P_, seed=5):
    P = O.init_params(_hp(P_), seed=seed)
    gen = torch.Generator().manual_seed(seed + 100)
    for k in P:
        if "layer_norm" in k:
            P[k] = P[k] + 0.1 * torch.randn(P[k].shape, generator=gen)
    return P


@functools.lru_cache(maxsize=None)
def _train_case():
    P_ = 2
    P = _params(P_)
    na = list(NA_B)
    c = SimpleNamespace(P=P, P_=P_, hp=_hp(P_), na=na, B=len(na), N=sum(na), m=_module(P_, P=P, sigmas_norm=_sigmas_norm()), fs=R.build_set(na, seed=23))
    c.tables, c.freqs = _tables(c.m), c.m.time_embedding.freqs.cpu()
    c.times = np.random.default_rng(len(na)).integers(1, T + 1, size=c.B).astype(np.int32)
    c.times[0], c.times[1] = 1, T
    c.nz = R.noise(c.fs, seed=60)
    c.y = np.array([[0.37, -1.5], [2.0, np.nan], [-0.8, 0.1], [11.5, 3.0], [np.nan, -2.2]])
    c.yhat, c.have = np.nan_to_num(c.y).astype(np.float32), np.isfinite(c.y).astype(np.int32)
    c.drop = GR.drop_mask(SEED, CALL, c.B, 0.5)
    assert c.drop.tolist() == [True, False, True, True, False]
    c.ref = GR.training_step(c.hp, P, c.tables, c.fs, c.nz, torch.float32, c.times, c.yhat, c.have, c.drop, F, c.freqs, grad=True)   # once, left unchanged
    return c


def _latent_grad(m, flat):
    return TA._grads(m, flat)["atom_latent_emb.weight"][:, 64 + 256:]


def test_conditional_micro_step_vs_oracle_autograd():
    from matinvent_amd import guidance, pretrain
    c = _train_case()
    assert np.array_equal(guidance.drop_mask(SEED, CALL, c.B, 0.5), c.drop)
    grad, stats = torch.zeros_like(c.m.decoder.theta), torch.zeros(4, device="cuda")
    pretrain.train_step(c.m, _ns(c.fs), c.times, noise=c.nz, grad=grad, stats=stats, seed=SEED, call_id=CALL, y=c.y, p_uncond=0.5)
    _grads_close(c.m, grad, c.ref["grads"], "fused conditional")
    _stats_close(stats, c.ref["stats"], "fused conditional")
    assert float(_latent_grad(c.m, grad).abs().max()) > 0
    # the unfused yardstick: training_step + autograd under the same mask
    c.m.decoder.theta.grad = None
    loss, d = c.m.training_step(_ns(c.fs), times=c.times, noise=c.nz, y=c.y, drop=c.drop)
    loss.backward()
    _grads_close(c.m, c.m.decoder.theta.grad, c.ref["grads"], "training_step")
    _stats_close(torch.stack([d[k].detach() for k in PR.STATS]), c.ref["stats"], "training_step")
    c.m.decoder.theta.grad = None
    # every crystal dropped: the latent columns see exact zeros, their gradient is exactly zero
    g1 = torch.zeros_like(grad)
    pretrain.train_step(c.m, _ns(c.fs), c.times, noise=c.nz, grad=g1, seed=SEED, call_id=CALL, y=c.y, p_uncond=1.0)
    assert torch.count_nonzero(_latent_grad(c.m, g1)) == 0 and float(g1.abs().max()) > 0
    g2 = torch.zeros_like(grad)
    pretrain.train_step(c.m, _ns(c.fs), c.times, noise=c.nz, grad=g2, seed=SEED, call_id=CALL, y=None)
    assert torch.equal(g1, g2)


def test_conditional_shards_and_pooled_handle():
    from matinvent_amd import pretrain
    from matinvent_amd.pool import HandlePool
    c = _train_case()
    kw = dict(seed=SEED, call_id=CALL, b_global=c.B, n_global=c.N, p_uncond=0.5)
    g0, s0 = torch.zeros_like(c.m.decoder.theta), torch.zeros(4, device="cuda")
    pretrain.train_step(c.m, _ns(c.fs), c.times, grad=g0, stats=s0, y=c.y, **kw)
    g1, s1 = torch.zeros_like(g0), torch.zeros(4, device="cuda")
    for idx, offsets in (([0, 1], (0, 0)), ([2, 3, 4], (8, 2))):
        pretrain.train_step(c.m, _ns(PR.subset(c.fs, idx)), c.times[idx], grad=g1, stats=s1, offsets=offsets, y=c.y[idx], **kw)
    _grads_close(c.m, g1, {"decoder." + k: v.cpu() for k, v in TA._grads(c.m, g0).items()}, "shards")
    _stats_close(s1, s0, "shards")
    pool = HandlePool()
    try:
        g2, s2 = torch.zeros_like(g0), torch.zeros(4, device="cuda")
        pretrain.train_step(c.m, _ns(c.fs), c.times, grad=g2, stats=s2, y=c.y, pool=pool, **kw)
        torch.cuda.synchronize()
        assert torch.equal(g2, g0) and torch.equal(s2, s0)
    finally:
        pool.close()


# ---- (4), (5) the guided chain ----------------------------------------------------------------------------------------------------------

CH_T, CH_SEED = 12, 4242
CH_NA = torch.tensor([4, 7, 2, 5])
CH_Y = np.array([0.37, -1.2, 2.5, np.nan])


@functools.lru_cache(maxsize=None)
def _chain_case(zero_latent=False):
    from matinvent_amd.guidance import Guidance
    hp = _hp(1)
    P = O.init_params(hp, seed=1, head_scale=0.1)
    if zero_latent:
        P["decoder.atom_latent_emb.weight"][:, 64 + 256:] = 0
    torch.manual_seed(99)
    m = _module(1, T_=CH_T, P=P)
    sn = torch.cat([torch.ones(1), 0.5 + torch.rand(CH_T)])
    m.sigma_scheduler.sigmas_norm.copy_(sn)
    c = SimpleNamespace(hp=hp, P=P, m=m, sch=O.Schedules.make(CH_T, sigmas_norm=sn), noise=O.philox_sampler_noise(CH_SEED, CH_NA, CH_T))
    c.g = lambda gamma: Guidance({"density": CH_Y}, gamma)
    c.yhat, c.have = np.nan_to_num(CH_Y).astype(np.float32)[:, None], np.isfinite(CH_Y).astype(np.int32)[:, None]
    return c


def _close(final, ref, tol):
    assert wrap_dist(final["frac_coords"].cpu().numpy(), ref["frac_coords"].numpy()).max() < tol
    np.testing.assert_allclose(final["lattices"].cpu().numpy(), ref["lattices"].numpy(), rtol=tol, atol=tol)
    np.testing.assert_allclose(final["atom_types"].cpu().numpy(), ref["atom_types"].numpy(), rtol=tol, atol=tol)


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("frac_coords", "lattices", "atom_types"))


@pytest.mark.parametrize("gamma", [0.0, 1.0])
def test_guided_chain_vs_reference_chain(gamma):
    c = _chain_case()
    ref, _ = GR.guided_chain(c.P, c.hp, c.sch, CH_NA, c.noise, torch.from_numpy(c.yhat), c.have, F, gamma)
    final, _ = c.m.sample(Box(CH_NA), step_lr=5e-6, seed=CH_SEED, guidance=c.g(gamma), streams=1)
    _close(final, ref, (1 + 2 * gamma) * 3e-4)
    if gamma == 0.0:   # ... and a property-conditioned module without guidance samples under the null row
        null, _ = GR.guided_chain(c.P, c.hp, c.sch, CH_NA, c.noise, None, None, F, 0.0)
        plain, _ = c.m.sample(Box(CH_NA), step_lr=5e-6, seed=CH_SEED, streams=1)
        _close(plain, null, 3e-4)


def test_zero_latent_columns_make_every_chain_the_same_chain():
    c = _chain_case(zero_latent=True)
    run = lambda **kw: c.m.sample(Box(CH_NA), step_lr=5e-6, seed=CH_SEED, streams=1, **kw)[0]
    plain, g0, g3 = run(), run(guidance=c.g(0.0)), run(guidance=c.g(3.0))
    assert _same(g3, g0) and _same(g0, plain)


def test_chains_differ_streams_agree_and_guidance_is_cleared():
    c = _chain_case()
    run = lambda **kw: c.m.sample(Box(CH_NA), step_lr=5e-6, seed=CH_SEED, **kw)[0]
    before = run(streams=1)
    g0, g3 = run(streams=1, guidance=c.g(0.0)), run(streams=1, guidance=c.g(3.0))
    after = run(streams=1)
    assert _same(before, after)                                                        # guidance was cleared from the cached handles
    assert not _same(g0, before) and not _same(g3, g0) and not _same(g3, before)
    two = run(streams=2, guidance=c.g(3.0))
    assert wrap_dist(two["frac_coords"].cpu().numpy(), g3["frac_coords"].cpu().numpy()).max() < 1e-4
    np.testing.assert_allclose(two["lattices"].cpu().numpy(), g3["lattices"].cpu().numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(two["atom_types"].cpu().numpy(), g3["atom_types"].cpu().numpy(), rtol=1e-4, atol=1e-4)
    assert _same(run(streams=2), run(streams=2)) and not _same(two, run(streams=2))


def test_guided_chain_on_a_respaced_view_equals_its_steps_walked_one_by_one():
    c = _chain_case()
    v = c.m.respaced(4)
    g = c.g(2.0)
    kw = dict(step_lr=5e-6, seed=CH_SEED, streams=1, guidance=g)
    full, _ = v.sample(Box(CH_NA), **kw)
    st, _ = v.sample(Box(CH_NA), t_start=4, t_stop=4, **kw)
    for k in range(4, 0, -1):
        st, _ = v.sample(Box(CH_NA), t_start=k, t_stop=k - 1, init=(st["frac_coords"], st["lattices"], st["atom_types"]), **kw)
    assert _same(st, full)
    assert not _same(full, c.m.sample(Box(CH_NA), **kw)[0])


# ---- (6) refusals -------------------------------------------------------------------------------------------------------------------------

def test_every_entry_that_fills_the_time_embedding_alone_refuses_a_latent_net():
    from matinvent_amd import _lib
    lib = _lib.load()
    m = _chain_case().m
    tables = {**_lib.PRETRAIN_SIGNATURES, **_lib.SIGNATURES, **_lib.TRAJ_SIGNATURES, **_lib.PG_SIGNATURES, **_lib.PG_KL_SIGNATURES, **_lib.DPO_SIGNATURES}
    for name in ("mi_pretrain_micro_step", "mi_ft_micro_step", "mi_ft_micro_steps_stacked", "mi_traj_logprob", "mi_traj_pg_step", "mi_traj_pg_kl_step",
                 "mi_dpo_micro_step"):
        args = []
        for k, ty in enumerate(tables[name][1]):   # the net first, nothing else: the refusal is the entry's first line
            args.append(m.decoder._h if k == 0 else 0.0 if ty is C.c_float else 0 if ty in (C.c_int, C.c_int64, C.c_uint64, C.c_uint32) else None)
        assert getattr(lib, name)(*args) == _lib.MI_EINVAL, name
        assert b"mi_net_set_latent" in lib.mi_last_error() and name.encode() in lib.mi_last_error(), name


def test_the_sampler_and_the_attach_refuse_before_anything_is_enqueued():
    from matinvent_amd import _lib, guidance, resampling
    from matinvent_amd.conditioning import Condition
    from matinvent_amd.pool import HandlePool
    lib = _lib.load()
    c = _chain_case()
    m = c.m
    na = [int(v) for v in CH_NA]
    cb, partner = m.make_batch(na), m.make_batch(na)
    yh, hv = c.yhat.copy(), c.have.copy()

    def refused(match, **kw):
        with pytest.raises(_lib.MIError, match=match) as e:
            m._sample_one(cb, 5e-6, CH_SEED, None, None, kw.get("record", False), None, 0, 0, 0)
        assert e.value.code == _lib.MI_EINVAL
    try:
        guidance.attach(cb, partner, yh, hv, F, 1.0)
        refused("record", record=True)
        guidance.attach(cb, partner, yh, hv, 4, 1.0)
        refused("F = 4")
        guidance.attach(cb, partner, np.concatenate([yh, yh], 1), np.concatenate([hv, hv], 1), F, 1.0)
        refused("P = 2")
        guidance.attach(cb, partner, yh, hv, F, 1.0)
        cond = Condition.composition([{"Na": 2, "Cl": 2}, {"Si": 7}, {"C": 2}, {"Fe": 5}], 4)
        cond.attach(m, cb)
        refused("replacement condition")
        Condition.clear(cb)
        cond.attach_likelihood(m, cb)
        refused("likelihood mask")
        Condition.clear_likelihood(cb)
        m.keep_lattice = True
        refused("CSP")
        m.keep_lattice = False
        # resampling: (1, j) is the plain chain for mi_sampler_run's resampling check, so the guidance check is what refuses it;
        # r = 2 without a condition is refused by the resampling check in front of it
        resampling.attach(m, cb, 1, 1)
        refused("guidance and resampling")
        resampling.attach(m, cb, 2, 1)
        refused("resampling .r = 2. and no condition")
        resampling.clear(cb)
        m._sample_one(cb, 5e-6, CH_SEED, None, None, False, None, 0, 0, 0)   # ... and with everything else cleared the guided chain runs
        # the attach itself
        for bad, match in (((cb, cb, yh, hv, F, 1.0), "partner"), ((cb, None, yh, hv, F, 1.0), "partner"), ((cb, m.make_batch(na[:3]), yh[:3], hv[:3], F, 1.0), "partner"),
                           ((cb, m.make_batch(na, 3, 1), yh, hv, F, 1.0), "partner"), ((cb, partner, yh, hv, 13, 1.0), "F = 13"),
                           ((cb, partner, yh, hv, F, float("inf")), "finite")):
            with pytest.raises(_lib.MIError, match=match) as e:
                guidance.attach(*bad)
            assert e.value.code == _lib.MI_EINVAL
        pool = HandlePool()
        pooled = m.make_batch(na, pool=pool)
        try:
            with pytest.raises(_lib.MIError, match="pooled") as e:
                guidance.attach(pooled, partner, yh, hv, F, 1.0)
            assert e.value.code == _lib.MI_EINVAL
        finally:
            pooled.release()
            pool.close()
    finally:
        guidance.clear(cb)
        resampling.clear(cb)
        m.keep_lattice = False
    # a net without a property part
    hp0 = O.CSPNetHParams(hidden_dim=64, num_layers=2, num_freqs=8)
    m0 = make_module(64, 2, 8, CH_T, O.init_params(hp0, seed=1, head_scale=0.1))
    cb0 = m0.make_batch(na)
    guidance.attach(cb0, m0.make_batch(na), yh, hv, F, 1.0)
    with pytest.raises(_lib.MIError, match="no property part") as e:
        m0._sample_one(cb0, 5e-6, CH_SEED, None, None, False, None, 0, 0, 0)
    assert e.value.code == _lib.MI_EINVAL
    guidance.clear(cb0)
    # mi_net_set_latent: the time part must stay a positive even number of columns
    assert lib.mi_net_set_latent(m0.decoder._h, 16, 8) == _lib.MI_EINVAL and b"positive even" in lib.mi_last_error()
    assert lib.mi_net_set_latent(m0.decoder._h, 1, 13) == _lib.MI_EINVAL
    assert lib.mi_net_latent_dim(m0.decoder._h) == 0 and lib.mi_net_latent_dim(m.decoder._h) == 2 * F


# ---- (7) end to end -----------------------------------------------------------------------------------------------------------------------

def test_fit_with_a_condition_learns_to_read_it_and_round_trips_through_load_model(tmp_path):
    """32 cubic crystals of 2-6 atoms whose cell edge is 6 + 1.5 y: the lattice is a function of the property, so the lattice loss under
    the property must fall below the lattice loss under the null condition."""
    from matinvent_amd import pretrain
    from matinvent_amd.data import CrystalData
    from matinvent_amd.suite import DiffCSPSuite
    g = torch.Generator().manual_seed(3)
    data = []
    for i in range(32):
        n = 2 + i % 5
        y = -2.0 + 4.0 * i / 31
        data.append(CrystalData(torch.rand(n, 3, generator=g), torch.randint(1, 90, (n,), generator=g), torch.full((1, 3), 6 + 1.5 * y),
                                torch.full((1, 3), 90.0), properties={"edge_y": y}))
    hparams = dict(decoder=dict(hidden_dim=64, num_layers=2, num_freqs=8), beta_scheduler=dict(timesteps=20), sigma_scheduler=dict(timesteps=20),
                   latent_dim=2 * F, condition=dict(properties=["edge_y"], num_freqs=F))
    suite = DiffCSPSuite("diffcsp", {"batch_size": 3, "num_batches": 1}, {"batch_size": 2}, random_init=True, head_scale=0.1, hparams=hparams, device="cuda:0")
    m = suite.load_model()
    for p in m.parameters():
        p.requires_grad = True
    cfg = dict(lr=2e-3, epochs=60, batch_size=8, handle_pool=True, condition=dict(properties=["edge_y"], num_freqs=F, p_uncond=0.2))
    hist = pretrain.fit(m, data, cfg, seed=SEED, log=lambda *_: None)
    assert hist[-1]["train_loss"] < hist[0]["train_loss"]
    assert abs(m.hparams["condition"]["mean"][0]) < 1e-9 and abs(m.hparams["condition"]["std"][0] - np.std([d.properties["edge_y"] for d in data])) < 1e-9
    on, off = pretrain.evaluate(m, data, 8, seed=SEED), pretrain.evaluate(m, data, 8, seed=SEED, condition=False)
    print(f"loss_lattice with the condition {on['loss_lattice']:.6g}, under the null condition {off['loss_lattice']:.6g}")
    assert on["loss_lattice"] < off["loss_lattice"], (on, off)
    suite.save_model(m, str(tmp_path / "cond"))
    m2 = DiffCSPSuite("diffcsp", {"batch_size": 3, "num_batches": 1}, {"batch_size": 2}, model_path=str(tmp_path / "cond"), device="cuda:0").load_model()
    assert m2.hparams["condition"] == m.hparams["condition"] and m2.normalizer.to_dict() == m.normalizer.to_dict()
    assert pretrain.evaluate(m2, data, 8, seed=SEED) == on and pretrain.evaluate(m2, data, 8, seed=SEED, condition=False) == off
    # a guided sample of the trained model runs end to end
    from matinvent_amd.guidance import Guidance
    final, _ = m2.sample(Box([3, 5, 2]), seed=1, guidance=Guidance({"edge_y": 1.0}, 2.0))
    assert all(bool(torch.isfinite(final[k]).all()) for k in ("atom_types", "frac_coords", "lattices"))

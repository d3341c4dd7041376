"""GPU checks of predictor-steered sampling (matinvent_amd/csrc/steer.hip under include/matinvent_hip_steer.h; matinvent_amd.steering;
the noise-aware additions of matinvent_amd.predictor).

(1) The plan kernel against tests/steer_ref.py.  (G, K) in {(1,1), (3,2), (5,5), (2,64), (1,256), (300,4)}: one particle, a partial wave,
one whole wave, four trips of the per-lane loops, 300 workgroups and a second trip of the statistics block's loop.  Ancestors, u_prev,
logw and the counts must EQUAL the reference for every group whose float64 thresholds lie further than 1e-4 * sum w from every cumulative
boundary (and whose ESS lies further than 1e-4 * K from its limit).  The margin is derived, not measured: the stored scores and
log-weights are the same bits as the reference's (separately rounded fp32 operations); the weights expf(lw - max) carry the subtraction's
rounding (at most 2^-24 * 16 relative for a weight above 1e-7) and a 2-ulp expf; sequential fp32 sums of at most 256 weights in [0, 1]
add at most K * 2^-24 of the sum: under (K + 4) * 2^-24 <= 1.6e-5 of sum w, a sixth of the margin.  No group is excluded: the seeds are
chosen on the CPU, with the oracle's Philox, so that the reference alone finds every group safe -- asserted first.
(2) The gather on [1, 2, 171, 20, 3] x 3 with node / graph offsets and NaN guard rows.  (3) mi_scalar_forward_state on g15's weights
against scalar_ref float32 at 2e-5 of max(1, |ref|), the bound DESIGN 42 holds mi_scalar_forward to.  (4) mi_scalar_micro_step_noised
against float32 autograd on the noised inputs at 2e-5 of max|ref| per tensor.  (5) The steered chain against the same schedule walked
with public pieces, bit for bit.  Nothing statistical is asserted."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import diffcsp_oracle as O
from tests import scalar_ref as SR
from tests import steer_ref as R
from tests.test_gpu_ft_arithmetic import _all
from tests.test_gpu_scalar import HEAD_SLICES, LOOP_NA, _close, _dev_grads, _g15, _hp, _model, _ns, _P, _targets
from tests.test_gpu_train import _rel

pytestmark = pytest.mark.gpu

L, F, TD, T = 2, 8, 256, 20
PLAN_CASES = [(1, 1), (3, 2), (5, 5), (2, 64), (1, 256), (300, 4)]
GATHER_NA = [1, 2, 171, 20, 3]


def _lib_():
    from matinvent_amd import _lib
    return _lib, _lib.load()


def _cuda(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to("cuda", dtype).contiguous()


def _resample(handle, K, out, p, mode, target, lam, ess_frac, seed, level, u_prev, logw, src, dst, anc, stats):
    from matinvent_amd.cspnet import _ptr, _stream
    _lib, lib = _lib_()
    rc = lib.mi_steer_resample(handle._h, K, _ptr(out), out.shape[1], p, mode, target, lam, ess_frac, seed, level, _ptr(u_prev), _ptr(logw),
                               _ptr(src[2]), _ptr(src[0]), _ptr(src[1]), _ptr(dst[2]), _ptr(dst[0]), _ptr(dst[1]), _ptr(anc), _ptr(stats), _stream())
    return rc, lib.mi_last_error().decode()


def _state(N, B, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(N, 3, generator=g).cuda(), torch.randn(B, 3, 3, generator=g).cuda(), torch.randn(N, 100, generator=g).cuda())


# ---- (1) the plan kernel ------------------------------------------------------------------------------------------------------------------

def _plan_inputs(G, K, seed, special=True):
    """out [B][2] (property 1 is read), u_prev, logw: NaN / +-inf scores, NaN previous scores, -inf log-weights, and (G >= 2) group 1 all NaN."""
    rng = np.random.default_rng([77, G, K, seed])
    B = G * K
    spread = 1.0 if K <= 64 else 4.0   # (256 particles: a few carry the weight, so that the boundaries are few enough for a safe seed to exist)
    out = (spread * rng.standard_normal((B, 2))).astype(np.float32)
    up = (spread * rng.standard_normal(B)).astype(np.float32)
    lg = (0.5 * rng.standard_normal(B)).astype(np.float32)
    if special and K >= 2:
        # (two particles: no special member besides the all-NaN group -- one survivor of two has ESS = 1 = 0.5 K exactly, on the limit)
        for g in range(0, G if K >= 4 else 0, 2):
            k = g * K + rng.integers(0, K, 3)
            out[k[0], 1], out[k[1], 1] = np.nan, (np.inf if g % 4 == 0 else -np.inf)
            up[g * K + rng.integers(0, K)] = np.nan
            lg[k[2]] = -np.inf
        if G >= 2:
            out[K:2 * K, 1] = np.nan
    return out, up, lg


@functools.lru_cache(maxsize=None)
def _plan_case(G, K, mode, ess_frac):
    """The case and its float64 reference, computed once, with the first seed under which the reference finds every group safe."""
    target, lam, level = 0.3, 1.5, 6
    for seed in range(400):
        out, up, lg = _plan_inputs(G, K, seed)
        U = R.uniforms(seed, level, G, K, graph_offset=0)
        ref = R.plan(out, 1, mode, target, lam, ess_frac, K, up, lg, U)
        if ref["safe"].all():
            return SimpleNamespace(seed=seed, out=out, up=up, lg=lg, U=U, ref=ref, target=target, lam=lam, level=level)
    return None


def test_the_shapes_reach_what_they_are_chosen_for():
    assert {K for _, K in PLAN_CASES} >= {1, 2, 5, 64, 256} and max(G for G, _ in PLAN_CASES) > 256
    c = _plan_case(300, 4, R.MODE_MAX, 0.5)
    assert c is not None and set(c.ref["flags"].tolist()) >= {0, R.RESAMPLED, R.NO_FINITE}   # groups that keep, resample and have no weight


@pytest.mark.parametrize("ess_frac", [-1.0, 0.5])
@pytest.mark.parametrize("mode", [R.MODE_MAX, R.MODE_MIN, R.MODE_TARGET])
@pytest.mark.parametrize("G,K", PLAN_CASES)
def test_plan_kernel_equals_the_float64_reference(G, K, mode, ess_frac):
    _lib, lib = _lib_()
    from matinvent_amd.cspnet import _ptr, _stream
    c = _plan_case(G, K, mode, ess_frac)
    assert c is not None and c.ref["safe"].all(), "no seed under which the reference alone finds every group safe: the excluded share must be zero"
    m = _model(64, 1)
    B = G * K
    cb = m.make_batch([1] * B)
    # the uniform, read back from the library's own fill: draw 29, step = level, element = the group's first crystal
    Ud = torch.empty(B, device="cuda")
    _lib.check(lib.mi_philox_fill(c.seed, c.level, 29, 0, B, 1, _ptr(Ud), _stream()))
    assert np.array_equal(Ud.cpu().numpy()[::K], c.U)
    out, up, lg = _cuda(c.out), _cuda(c.up), _cuda(c.lg)
    src, dst = _state(B, B, 1), _state(B, B, 2)
    anc, stats = torch.full((B,), -7, dtype=torch.int32, device="cuda"), torch.tensor([10.0, 20.0, 30.0], device="cuda")
    rc, msg = _resample(cb, K, out, 1, mode, c.target, c.lam, ess_frac, c.seed, c.level, up, lg, src, dst, anc, stats)
    assert rc == 0, msg
    ref = c.ref
    assert np.array_equal(anc.cpu().numpy(), ref["ancestors"])
    assert np.array_equal(up.cpu().numpy(), ref["u_prev"], equal_nan=True) and np.array_equal(lg.cpu().numpy(), ref["logw"], equal_nan=True)
    st = stats.cpu().double().numpy() - [10.0, 20.0, 30.0]   # (+=: the prefilled values stay underneath)
    assert st[0] == ref["stats"][0] and st[2] == ref["stats"][2]
    assert abs(st[1] - ref["stats"][1]) <= 3 * (K + 4) * 2.0 ** -24 * max(1.0, ref["stats"][1]) + 2.0 ** -20 * 20.0   # (the last term: fp32 rounding of 20 + sum)
    rows = torch.as_tensor(ref["ancestors"]).cuda()
    assert torch.equal(dst[0], src[0][rows]) and torch.equal(dst[1], src[1][rows]) and torch.equal(dst[2], src[2][rows])
    cb.release()


@pytest.mark.parametrize("G,K", [(3, 2), (5, 5), (2, 64), (1, 256)])
def test_a_large_lambda_gives_every_group_its_arg_max(G, K):
    rng = np.random.default_rng([78, G, K])
    B = G * K
    while True:
        out = rng.standard_normal((B, 1)).astype(np.float32)
        top2 = np.sort(out.reshape(G, K), axis=1)[:, -2:]
        if np.all(top2[:, 1] - top2[:, 0] > 0.01):
            break
    m = _model(64, 1)
    cb = m.make_batch([1] * B)
    up, lg = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
    src, dst = _state(B, B, 1), _state(B, B, 2)
    anc = torch.empty(B, dtype=torch.int32, device="cuda")
    rc, msg = _resample(cb, K, _cuda(out), 0, R.MODE_MAX, 0.0, 1e4, -1.0, 5, 3, up, lg, src, dst, anc, None)
    assert rc == 0, msg
    best = (np.arange(G) * K + out.reshape(G, K).argmax(axis=1)).repeat(K)
    assert np.array_equal(anc.cpu().numpy(), best)
    assert np.array_equal(up.cpu().numpy(), out[best, 0]) and not lg.any()
    cb.release()


# ---- (2) the gather ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("guard", [32, 1])   # (32 floats: the 16-byte path of the type rows; 1 float: dst is not 16-byte aligned, the dword path)
def test_gather_moves_the_ancestors_rows_and_nothing_else(guard):
    K = 3
    na = [n for n in GATHER_NA for _ in range(K)]
    B, N = len(na), sum(na)
    m = _model(64, 1)
    cb = m.make_batch(na, 1000, 50)   # non-zero node and graph offsets: the uniform's element index is 50 + g K
    seed, level, lam = 4, 9, 2.0
    rng = np.random.default_rng(5)
    out = rng.standard_normal((B, 1)).astype(np.float32)
    U = R.uniforms(seed, level, len(GATHER_NA), K, graph_offset=50)
    ref = R.plan(out, 0, R.MODE_MIN, 0.0, lam, -1.0, K, np.zeros(B, np.float32), np.zeros(B, np.float32), U)
    assert ref["safe"].all() and not np.array_equal(ref["ancestors"], np.arange(B))
    src = _state(N, B, 3)
    keep = tuple(v.clone() for v in src)
    bufs = [torch.full((v.numel() + 2 * guard,), float("nan"), device="cuda") for v in src]
    dst = tuple(b[guard:guard + v.numel()].view(v.shape) for b, v in zip(bufs, src))
    anc = torch.empty(B, dtype=torch.int32, device="cuda")
    up, lg = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
    rc, msg = _resample(cb, K, _cuda(out), 0, R.MODE_MIN, 0.0, lam, -1.0, seed, level, up, lg, src, dst, anc, None)
    assert rc == 0, msg
    assert np.array_equal(anc.cpu().numpy(), ref["ancestors"])
    rows = torch.as_tensor(R.gather_rows(na, ref["ancestors"])).cuda()
    assert torch.equal(dst[0], src[0][rows]) and torch.equal(dst[2], src[2][rows]) and torch.equal(dst[1], src[1][torch.as_tensor(ref["ancestors"]).cuda()])
    for a, b in zip(src, keep):
        assert torch.equal(a, b)
    for b in bufs:
        assert torch.isnan(b[:guard]).all() and torch.isnan(b[-guard:]).all() and torch.isfinite(b[guard:-guard]).all()
    cb.release()


def test_resample_refusals_before_anything_is_enqueued():
    _lib, lib = _lib_()
    m = _model(64, 1)
    cb = m.make_batch([2, 2, 3, 3])
    B, N = 4, 10
    out, up, lg = torch.zeros(B, 2, device="cuda"), torch.full((B,), 0.5, device="cuda"), torch.full((B,), 0.25, device="cuda")
    src, dst = _state(N, B, 1), _state(N, B, 2)
    keep = tuple(v.clone() for v in dst)
    anc, stats = torch.full((B,), -7, dtype=torch.int32, device="cuda"), torch.zeros(3, device="cuda")

    def call(K=2, p=0, mode=0, target=0.0, lam=1.0, ess=-1.0, h=cb, s=src, d=dst):
        return _resample(h, K, out, p, mode, target, lam, ess, 1, 1, up, lg, s, d, anc, stats)

    def refused(rc_msg, text):
        assert rc_msg[0] == _lib.MI_EINVAL and text in rc_msg[1], rc_msg

    refused(call(K=0), "particles per group")
    refused(call(K=257), "particles per group")
    refused(call(K=3), "B % K != 0")
    refused(call(K=4), "share one atom count")
    refused(call(p=2), "property p = 2 of P = 2")
    refused(call(mode=3), "unknown mode")
    refused(call(lam=float("nan")), "lambda is not finite")
    refused(call(lam=float("inf")), "lambda is not finite")
    refused(call(ess=float("nan")), "ess_frac is not finite")
    refused(call(mode=2, target=float("inf")), "target_hat is not finite")
    refused(call(d=src), "dst aliases src")
    refused(call(d=(dst[0], src[1], dst[2])), "dst aliases src")   # (one of the three arrays is enough)
    torch.cuda.synchronize()
    assert (anc == -7).all() and not stats.any() and (up == 0.5).all() and (lg == 0.25).all() and all(torch.equal(a, b) for a, b in zip(dst, keep))
    assert call()[0] == 0 and (anc >= 0).all()
    cb.release()
    e = m.make_batch([])
    assert lib.mi_steer_resample(e._h, 2, None, 1, 0, 0, 0.0, 1.0, -1.0, 0, 0, *([None] * 11)) == 0   # B = 0: MI_OK, nothing launched
    e.release()


# ---- (3) the forward on a state -------------------------------------------------------------------------------------------------------------

def _noisy_state(fs, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    na = fs["num_atoms"]
    N, B = int(na.sum()), len(na)
    _, onehot, fr, lat = SR.clean_inputs(fs["atom_types"], fs["frac"], fs["lengths"], fs["angles"], torch.zeros(B), TD, dtype)
    types = 0.8 * onehot + 0.3 * torch.randn(N, 100, generator=g).to(dtype)
    frac = (fr + 0.1 * torch.randn(N, 3, generator=g).to(dtype)) % 1.0
    return types, frac, lat + 0.2 * torch.randn(B, 3, 3, generator=g).to(dtype)


def test_forward_state_vs_scalar_ref_on_the_reference_fixture(golden):
    from matinvent_amd import predictor as PR
    m, P, fs = _g15(golden)
    na = fs["num_atoms"].tolist()
    cb = m.make_batch(na)
    types, frac, lat = _noisy_state(fs, 3)
    state = dict(atom_types=types.cuda(), frac_coords=frac.cuda(), lattices=lat.cuda())
    keep = {k: v.clone() for k, v in state.items()}
    temb = lambda times: O.time_embedding(torch.tensor(times).long(), TD).float()
    reft, ref5 = (SR.forward(P, _hp(64), temb(t), types, frac, lat, fs["num_atoms"])[0] for t in ([3, 0, 17], [5, 5, 5]))
    clean = SR.forward(P, _hp(64), temb([3, 0, 17]), *SR.clean_inputs(fs["atom_types"], fs["frac"], fs["lengths"], fs["angles"], torch.zeros(3), TD, torch.float32)[1:],
                       fs["num_atoms"])[0]
    assert float((reft - clean).abs().min()) > 1e-3   # the noise is seen
    _close(PR.forward_state(m, state, cb, torch.tensor([3, 0, 17])), reft, 2e-5, "forward_state at times [3, 0, 17]")
    o5 = PR.forward_state(m, state, cb, 5)
    _close(o5, ref5, 2e-5, "forward_state at t_all = 5")
    assert torch.equal(PR.forward_state(m, (state["frac_coords"], state["lattices"], state["atom_types"]), cb, torch.tensor([5, 5, 5])), o5)
    assert all(torch.equal(state[k], keep[k]) for k in state)
    # a clean state at time 0 against mi_scalar_forward
    _, onehot, fr, lt = SR.clean_inputs(fs["atom_types"], fs["frac"], fs["lengths"], fs["angles"], torch.zeros(3), TD, torch.float32)
    o0 = PR.forward_state(m, dict(atom_types=onehot.cuda(), frac_coords=fr.cuda(), lattices=lt.cuda()), cb, 0)
    _close(o0, PR.forward(m, _ns(fs)).cpu(), 2e-5, "forward_state on a clean state at time 0 vs mi_scalar_forward")
    # refusals: mi_scalar_forward's, and the shapes
    _lib, lib = _lib_()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    tm = np.array([0, 1, 2], np.int32)
    _lib.check(lib.mi_batch_set_time_map(cb._h, ip(tm), 3))
    with pytest.raises(_lib.MIError, match="time map"):
        PR.forward_state(m, state, cb, 0)
    _lib.check(lib.mi_batch_set_time_map(cb._h, None, 0))
    with pytest.raises(ValueError, match="not the handle's"):
        PR.forward_state(m, dict(state, frac_coords=state["frac_coords"][1:]), cb, 0)
    from matinvent_amd.cspnet import _ptr, _stream
    _, W, bias = m.head_slices()
    rc = lib.mi_scalar_forward_state(m.trunk._h, cb._h, _ptr(state["atom_types"]), _ptr(state["frac_coords"]), _ptr(state["lattices"]),
                                     _ptr(m.time_freqs), None, 0, _ptr(W), _ptr(bias), 0, _ptr(o5), _stream())
    assert rc == _lib.MI_EINVAL and b"at least 1" in lib.mi_last_error()
    cb.release()


# ---- (4) the noised micro-step -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _diffusion():
    from tests.gpu_util import make_module
    return make_module(64, L, F, T, sigmas_norm=torch.linspace(0.7, 1.3, T + 1))


def _noised_inputs(fs, times, noise, dtype):
    """The forward noising of mi_add_noise_per_crystal on the host: c0 L + c1 z_l, (x + sigma z_x) % 1, c0 onehot + c1 z_t."""
    from matinvent_amd.pretrain import schedule_table
    tab = schedule_table(_diffusion()).cpu().to(dtype)[torch.as_tensor(times).long()]
    na = fs["num_atoms"]
    t_emb, onehot, fr, lat = SR.clean_inputs(fs["atom_types"], fs["frac"], fs["lengths"], fs["angles"], torch.as_tensor(times), TD, dtype)
    zl, zx, zt = (v.to(dtype) for v in noise)
    a = lambda v: v.repeat_interleave(na)[:, None]
    return (t_emb, a(tab[:, 0]) * onehot + a(tab[:, 1]) * zt, (torch.as_tensor(fs["frac"]).to(dtype) + a(tab[:, 2]) * zx) % 1.0,
            tab[:, 0, None, None] * lat + tab[:, 1, None, None] * zl.view(-1, 3, 3))


@functools.lru_cache(maxsize=None)
def _noised_case(P, kind):
    m = _model(64, P)
    fs = SR.build_set(LOOP_NA, seed=43)
    B, N = len(LOOP_NA), sum(LOOP_NA)
    g = torch.Generator().manual_seed(44)
    c = SimpleNamespace(m=m, fs=fs, B=B, N=N, ACC=2, kind=kind, times=[0, T, 7, 3, 12], tg=_targets(B, P, seed=17),
                        noise=(torch.randn(B, 9, generator=g), torch.randn(N, 3, generator=g), torch.randn(N, 100, generator=g)))
    c.ins = _noised_inputs(fs, c.times, c.noise, torch.float32)
    c.ref = SR.micro_step(_P(m), _hp(64), *c.ins, fs["num_atoms"], *c.tg, kind=kind, accum=c.ACC)   # computed once, left unchanged
    return c


@pytest.mark.parametrize("P,kind", [(3, "mse"), (1, "l1")])
def test_noised_micro_step_vs_float32_autograd_on_the_noised_inputs(P, kind):
    from matinvent_amd import predictor as PR
    c = _noised_case(P, kind)
    m, d = c.m, _diffusion()
    yhat, have, cg = c.tg
    kw = dict(yhat=yhat, have=have, count_global=cg, accum_steps=c.ACC, loss=kind)
    cb = m.make_batch(LOOP_NA)
    pattern = torch.full_like(m.flat, 0.375)
    grad, stats, out = pattern.clone(), torch.zeros(PR.stats_len(P), device="cuda"), torch.empty(c.B, P, device="cuda")
    PR.train_step_noised(m, _ns(c.fs), c.times, d, noise=c.noise, grad=grad, stats=stats, out=out, handle=cb, **kw)
    for k, g in _dev_grads(m, grad).items():   # the three diffusion heads' slices: the prefilled pattern, bit for bit
        if k[len("decoder."):] in HEAD_SLICES:
            assert torch.equal(g, torch.full_like(g, 0.375)), k
    gz = grad - pattern
    for k, g in _dev_grads(m, gz).items():
        if k[len("decoder."):] not in HEAD_SLICES:
            _rel(g, c.ref["grads"][k].numpy(), 2e-5, f"noised P={P} {kind}: grad {k}")
    _close(out, c.ref["out"], 2e-5, "noised taped form: out")
    # the statistics: the head on the device's own features in float64, within 4 x the float32 formulas' own deviation
    hf = m.trunk.tap(cb, L + 1).cpu()
    _, W, bias = (v.detach().cpu() for v in m.head_slices())
    r = {dt: SR.stats(SR.head(SR.pooled(hf.to(dt), LOOP_NA), W.view(P, 64).to(dt), bias.to(dt)), yhat, have, cg, kind) for dt in (torch.float64, torch.float32)}
    _all([((stats[k:k + 1], r[torch.float64][k:k + 1], r[torch.float32][k:k + 1], f"noised stats[{k}]"), {}) for k in range(PR.stats_len(P))])
    # the forward-only form: same outputs up to the inference forward's rounding, same statistics' counts, no gradient
    o2, s2 = torch.empty(c.B, P, device="cuda"), torch.zeros(PR.stats_len(P), device="cuda")
    PR.train_step_noised(m, _ns(c.fs), c.times, d, noise=c.noise, stats=s2, out=o2, handle=cb, forward_only=True, **kw)
    _close(o2, c.ref["out"], 2e-5, "noised forward-only form: out")
    _rel(s2, c.ref["stats"].numpy(), 1e-4, "noised forward-only form: statistics")
    assert s2[3::3].tolist() == have.sum(axis=0).tolist()
    # at time 0 for every crystal the micro-step is mi_scalar_micro_step's: the clean row (1, 0, 0, .)
    o3, o4 = torch.empty(c.B, P, device="cuda"), torch.empty(c.B, P, device="cuda")
    PR.train_step_noised(m, _ns(c.fs), [0] * c.B, d, noise=c.noise, out=o3, handle=cb, forward_only=True, **kw)
    PR.train_step(m, _ns(c.fs), out=o4, handle=cb, forward_only=True, **kw)
    _close(o3, o4.cpu(), 2e-5, "noised form at time 0 vs the clean form")
    cb.release()


def test_device_draws_equal_the_injected_host_philox_draws():
    from matinvent_amd import predictor as PR
    c = _noised_case(3, "mse")
    m, d = c.m, _diffusion()
    yhat, have, cg = c.tg
    kw = dict(yhat=yhat, have=have, count_global=cg, accum_steps=c.ACC, loss="mse")
    seed, call, off = 21, 5, (40, 6)
    host = (torch.from_numpy(O.philox_normal(seed, call, 7, c.B * 9, off[1] * 9)).view(c.B, 9), torch.from_numpy(O.philox_normal(seed, call, 8, c.N * 3, off[0] * 3)).view(c.N, 3),
            torch.from_numpy(O.philox_normal(seed, call, 9, c.N * 100, off[0] * 100)).view(c.N, 100))
    res = []
    for noise in (None, host):
        grad, out = torch.zeros_like(m.flat), torch.empty(c.B, 3, device="cuda")
        PR.train_step_noised(m, _ns(c.fs), c.times, d, noise=noise, grad=grad, out=out, seed=seed, call_id=call, offsets=off, **kw)
        res.append((grad, out))
    _close(res[0][1], res[1][1].cpu(), 2e-5, "device draws vs injected host Philox: out")
    ref = _dev_grads(m, res[1][0])
    for k, g in _dev_grads(m, res[0][0]).items():
        if k[len("decoder."):] not in HEAD_SLICES:
            _rel(g, ref[k].cpu().numpy(), 2e-5, f"device draws vs injected host Philox: grad {k}")
    assert float(res[0][0].abs().max()) > 0


def test_noised_micro_step_refusals():
    from matinvent_amd import predictor as PR
    from matinvent_amd.cspnet import _ptr, _stream
    from matinvent_amd.pretrain import schedule_table
    _lib, lib = _lib_()
    c = _noised_case(3, "mse")
    m, d = c.m, _diffusion()
    yhat, have, cg = c.tg
    cb = m.make_batch(LOOP_NA)
    f = lambda x: x.cuda().float().contiguous()
    b = _ns(c.fs)
    lengths, angles, frac, at = f(b.lengths), f(b.angles), f(b.frac_coords), b.atom_types.cuda().int().contiguous()
    yd, hd, cgd = _cuda(yhat), _cuda(have, torch.int32), _cuda(cg, torch.int32)
    hv, cgh = np.ascontiguousarray(have, dtype=np.int32), np.ascontiguousarray(cg, dtype=np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    m.trunk.sync()
    _, W, bias = m.head_slices()
    grad, stats = torch.zeros_like(m.flat), torch.zeros(PR.stats_len(3), device="cuda")
    gt, gW, gb = m.head_slices(grad)
    table = schedule_table(d)

    def step(times, T_=T, P=3, accum=1):
        th = np.asarray(times, np.int32)
        rc = lib.mi_scalar_micro_step_noised(m.trunk._h, cb._h, _ptr(lengths), _ptr(angles), _ptr(frac), _ptr(at), _ptr(m.time_freqs), ip(th), _ptr(_cuda(th, torch.int32)),
                                             _ptr(table), T_, 1, 1, None, None, None, _ptr(W), _ptr(bias), P, _ptr(yd), _ptr(hd), ip(hv), _ptr(cgd), ip(cgh),
                                             accum, 0, _ptr(gt), _ptr(gW), _ptr(gb), _ptr(stats), None, _stream())
        return rc, lib.mi_last_error().decode()

    for times, text in (([0, 1, 2, 3, T + 1], f"t[4] = {T + 1}: a time lies in 0..T = {T}"), ([-1, 1, 2, 3, 4], "t[0] = -1")):
        rc, msg = step(times)
        assert rc == _lib.MI_EINVAL and text in msg, (rc, msg)
    for kw, text in ((dict(T_=0), "T = 0"), (dict(P=0), "at least 1"), (dict(accum=0), "accum_steps")):
        rc, msg = step([0, 1, 2, 3, 4], **kw)
        assert rc == _lib.MI_EINVAL and text in msg, (rc, msg)
    tm = np.array([0, 1, 2], np.int32)
    _lib.check(lib.mi_batch_set_time_map(cb._h, ip(tm), 3))
    rc, msg = step([0, 1, 2, 3, 4])
    assert rc == _lib.MI_EINVAL and "time map" in msg and "mi_scalar_micro_step_noised" in msg
    _lib.check(lib.mi_batch_set_time_map(cb._h, None, 0))
    torch.cuda.synchronize()
    assert not grad.any() and not stats.any()
    assert step([0, T, 2, 3, 4])[0] == 0 and torch.isfinite(grad).all() and grad.any()
    cb.release()


def test_fit_predictor_noised_on_a_toy_set_and_the_model_directory(tmp_path):
    """fit_predictor(diffusion=): times and noise are functions of (seed, epoch, step), so two runs give the same bits; hparams["noised"]
    is recorded and travels through the model directory; evaluate(t=) gives the error at a fixed time, and at t = 0 that of the clean
    evaluation up to the inference forward's rounding.  (A toy set and random crystals: nothing is claimed about the fit.)"""
    from matinvent_amd import predictor as PR, steering as ST
    from tests.test_gpu_scalar import _toy
    d = _diffusion()
    train, val = _toy(24, seed=1), _toy(8, seed=2)
    cfg = dict(lr=3e-3, epochs=3, batch_size=8, max_grad_norm=10.0, skip_nonfinite_steps=True, handle_pool=True)
    runs = []
    for _ in range(2):
        m = PR.PropertyPredictor(["zbar"], hidden_dim=64, num_layers=2, time_dim=256, num_freqs=8, ln=True, device="cuda", seed=3)
        assert m.noised is None
        hist = PR.fit_predictor(m, train, cfg, val_list=val, seed=4, log=lambda s: None, diffusion=d)
        runs.append((m, hist))
    (m, hist), (m2, hist2) = runs
    assert torch.equal(m.flat.data, m2.flat.data) and hist == hist2 and len(hist) == 3
    assert all(np.isfinite(h["train_loss"]) and np.isfinite(h["val_loss"]) for h in hist)
    assert m.noised == PR.noised_spec(d) and m.noised["T"] == T
    clean = PR.PropertyPredictor(["zbar"], hidden_dim=64, num_layers=2, time_dim=256, num_freqs=8, ln=True, device="cuda", seed=3)
    PR.fit_predictor(clean, train, dict(cfg, epochs=1), seed=4, log=lambda s: None)
    assert clean.noised is None and not torch.equal(clean.flat.data, m.flat.data)
    e0, eT = PR.evaluate(m, val, 8, t=0, diffusion=d)["zbar"], PR.evaluate(m, val, 8, t=T, diffusion=d)["zbar"]
    ec = PR.evaluate(m, val, 8)["zbar"]
    assert e0["count"] == eT["count"] == 8 and np.isfinite(eT["mse"]) and abs(e0["mse"] - ec["mse"]) <= 1e-4 * max(ec["mse"], 1e-6) and eT["mse"] != e0["mse"]
    assert PR.evaluate(m, val, 8, t=7, diffusion=d, seed=5) == PR.evaluate(m, val, 8, t=7, diffusion=d, seed=5)
    path = PR.save_predictor(m, str(tmp_path / "noised"))
    q = PR.load_predictor(path, device="cuda", names=["zbar"])
    assert q.noised == m.noised and torch.equal(q.flat.data, m.flat.data)
    s = ST.Steering.from_config(dict(model_path=path, task="zbar", particles=2, every=5), device="cuda")
    from tests.gpu_util import Box
    final, _, info = d.sample(Box(s.replicate([3, 2])), seed=2, steer=s)
    assert info["levels"] == [15, 10, 5, 0] and torch.isfinite(final["lattices"]).all()


# ---- (5) the chain -------------------------------------------------------------------------------------------------------------------------

GROUPS, KP = [2, 5, 1], 4


@functools.lru_cache(maxsize=None)
def _chain():
    from matinvent_amd import predictor as PR
    mod = _diffusion()
    pred = PR.PropertyPredictor(["y"], hidden_dim=64, num_layers=L, time_dim=TD, num_freqs=F, ln=True, device="cuda", seed=12)
    pred.hparams["noised"] = PR.noised_spec(mod)
    return mod, pred


def _walk(view, steer, box, seed):
    """The steered chain with public pieces: sample(init=, t_start=, t_stop=) segments, forward_state, mi_steer_resample."""
    from matinvent_amd import predictor as PR, steering as ST
    S = view.beta_scheduler.timesteps
    tau = view.time_map.tolist() if view.time_map is not None else list(range(S + 1))
    na = box.num_atoms.tolist()
    B = len(na)
    tup = lambda f: (f["frac_coords"], f["lattices"], f["atom_types"])
    state = tup(view.sample(box, seed=seed, t_start=S, t_stop=S)[0])   # the initial draw, wrapped
    ph = steer.predictor.make_batch(na)
    u_prev, logw = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
    at, ancs, stats = S, [], []
    for k in steer.schedule(S):
        if k < at:
            state = tup(view.sample(box, seed=seed, init=state, t_start=at, t_stop=k)[0])
            at = k
        out = PR.forward_state(steer.predictor, state, ph, tau[k])
        dst = tuple(torch.empty_like(v) for v in state)
        anc, st = torch.empty(B, dtype=torch.int32, device="cuda"), torch.zeros(3, device="cuda")
        ST.resample(steer, ph, out, k, seed, u_prev, logw, state, dst, anc, st)
        state = dst
        ancs.append(anc.cpu())
        stats.append(st.cpu())
    if at > 0:
        state = tup(view.sample(box, seed=seed, init=state, t_start=at, t_stop=0)[0])
    ph.release()
    return state, torch.stack(ancs), torch.stack(stats)


@pytest.mark.parametrize("steps", [None, 6])
def test_steered_chain_equals_the_schedule_walked_with_public_pieces(steps):
    from matinvent_amd import steering as ST
    from tests.gpu_util import Box
    mod, pred = _chain()
    view = mod if steps is None else mod.respaced(steps)
    s = ST.Steering(pred, "y", mode="max", particles=KP, scale=3.0, every=2)
    box = Box(s.replicate(GROUPS))
    final, traj, info = view.sample(box, seed=7, steer=s)
    S = view.beta_scheduler.timesteps
    assert info["levels"] == list(range(S - 2, -1, -2)) and info["times"] == ([13, 7, 0] if steps else info["levels"]) and traj[0] is final
    state, ancs, stats = _walk(view, s, box, 7)
    assert torch.equal(final["frac_coords"], state[0]) and torch.equal(final["lattices"], state[1]) and torch.equal(final["atom_types"], state[2])
    assert torch.equal(info["ancestors"], ancs) and torch.equal(info["stats"], stats)
    B = len(GROUPS) * KP
    assert info["ancestors"].shape == (len(info["levels"]), B) and bool((info["ancestors"] // KP == torch.arange(B) // KP).all())
    assert info["stats"][:, 0].tolist() == [float(len(GROUPS))] * len(info["levels"]) and not info["stats"][:, 2].any()
    assert bool((info["stats"][:, 1] > 0).all()) and bool((info["stats"][:, 1] <= B + 1e-3).all())
    # two runs are the same bits
    f2, _, i2 = view.sample(box, seed=7, steer=s)
    assert all(torch.equal(final[k], f2[k]) for k in ("frac_coords", "lattices", "atom_types")) and torch.equal(info["ancestors"], i2["ancestors"])
    assert torch.isfinite(final["frac_coords"]).all() and torch.isfinite(final["lattices"]).all()


@pytest.mark.parametrize("steps", [None, 6])
def test_one_particle_and_a_zero_scale_leave_the_plain_chain(steps):
    from matinvent_amd import steering as ST
    from tests.gpu_util import Box
    mod, pred = _chain()
    view = mod if steps is None else mod.respaced(steps)
    same = lambda a, b: all(torch.equal(a[k], b[k]) for k in ("frac_coords", "lattices", "atom_types"))
    one = ST.Steering(pred, "y", particles=1, scale=3.0, every=2)
    plain1, _ = view.sample(Box(GROUPS), seed=9)
    f1, _, i1 = view.sample(Box(GROUPS), seed=9, steer=one)
    assert same(f1, plain1) and bool((i1["ancestors"] == torch.arange(len(GROUPS))).all())
    zero = ST.Steering(pred, "y", particles=KP, scale=0.0, every=2)
    box = Box(zero.replicate(GROUPS))
    plain4, _ = view.sample(box, seed=9)
    f4, _, i4 = view.sample(box, seed=9, steer=zero)
    assert same(f4, plain4) and bool((i4["ancestors"] == torch.arange(len(GROUPS) * KP)).all())
    assert i4["stats"][:, 0].tolist() == [float(len(GROUPS))] * i4["stats"].shape[0]   # (resampled, to the identity: equal weights by construction)


def test_particles_that_share_an_ancestor_differ_after_the_next_step():
    from matinvent_amd import steering as ST
    from tests.gpu_util import Box
    mod, pred = _chain()
    s = ST.Steering(pred, "y", particles=KP, scale=1e4, levels=[10])   # one event; the tilt is so steep that a group's particles take one ancestor
    na = s.replicate(GROUPS)
    box = Box(na)
    at10, _, info = mod.sample(box, seed=11, t_stop=10, steer=s)
    anc = info["ancestors"][0].view(len(GROUPS), KP)
    assert info["levels"] == [10] and bool((anc == anc[:, :1]).all())
    end, _, _ = mod.sample(box, seed=11, steer=s)
    off = np.concatenate([[0], np.cumsum(na)])
    for g in range(len(GROUPS)):
        rows = [slice(off[g * KP + k], off[g * KP + k + 1]) for k in range(KP)]
        for k in range(1, KP):
            assert torch.equal(at10["frac_coords"][rows[k]], at10["frac_coords"][rows[0]]) and torch.equal(at10["lattices"][g * KP + k], at10["lattices"][g * KP])
            assert not torch.equal(end["frac_coords"][rows[k]], end["frac_coords"][rows[0]])
            assert not torch.equal(end["lattices"][g * KP + k], end["lattices"][g * KP])


def test_generate_returns_the_replicated_records():
    from matinvent_amd import steering as ST
    from matinvent_amd.sampling import DiffCSPSampler
    mod, pred = _chain()
    s = ST.Steering(pred, "y", mode="target", target=0.1, particles=KP, scale=1.0, every=5, ess=0.5)
    smp = DiffCSPSampler(batch_size=3, num_batches=1)
    data, strucs = smp.generate(mod, steer=s)
    assert len(data) == len(strucs) == 3 * KP
    counts = [int(d.num_atoms) for d in data]
    assert counts == [c for c in counts[::KP] for _ in range(KP)]
    assert smp.last_steer["levels"] == [15, 10, 5, 0] and smp.last_steer["ancestors"].shape == (4, 3 * KP)

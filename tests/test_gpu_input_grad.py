"""GPU checks of classifier guidance (matinvent_amd/csrc/input_grad.hip under include/matinvent_hip_inputgrad.h; predictor.input_gradient;
matinvent_amd.classifier) against tests/input_grad_ref.py.

(1) The input gradient -- g_frac, g_lat, g_types -- against float32 autograd of tests/scalar_ref.forward at 2e-5 of max|ref| per tensor,
the project's gradient bound; next to it the ratio of the device's error to the float32 reference's own deviation from float64 autograd
is printed (MI_TOL_REPORT).  Shapes, one per code path: g15's weights at noisy inputs and times [3, 0, 17]; random weights H = 64, L = 2
at [1, 2, 171, 20, 3] (171 > 64: the non-fused pair path; 1: no pair); 300 crystals of 1-3 atoms (several blocks of every launch);
H = 512 at 30 x 20 (Np = 5700 >= 4096, E = 12000 >= 8192: the path whose weight gradient reads Dm / Dp as plane sets); P in {1, 3} with an
arbitrary d_out.  (2) mi_guide_seed and mi_guide_shift against the float64 reference.  (3) The sign, end to end.  (4) The chain against
the same schedule walked with public pieces, bit for bit.  Nothing statistical is asserted: the weights are random and there is no
dataset, so whether guidance moves a sampled property cannot be measured here; `scale` ships untuned."""
import ctypes as C
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import diffcsp_oracle as O
from tests import input_grad_ref as R
from tests import scalar_ref as SR
from tests.test_gpu_ft_arithmetic import _all
from tests.test_gpu_scalar import GRID_NA, LOOP_NA, _close, _dev_grads, _g15, _ns, _targets
from tests.test_gpu_steer import _noisy_state

pytestmark = pytest.mark.gpu

L, F, TD, T = 2, 8, 256, 20
BIG_NA = [20] * 30
GRAD_TOL = 2e-5   # of max|ref| per tensor: the project's gradient bound (tests/test_gpu_pretrain.py, tests/test_gpu_scalar.py)
FWD_TOL = 2e-5    # of max(1, |ref|): DESIGN 43's forward bound


def _lib_():
    from matinvent_amd import _lib
    return _lib, _lib.load()


@functools.lru_cache(maxsize=None)
def _diffusion():
    from tests.gpu_util import make_module
    return make_module(64, L, F, T, sigmas_norm=torch.linspace(0.7, 1.3, T + 1))


@functools.lru_cache(maxsize=None)
def _model(H, P, seed=21):
    """A noise-aware predictor of this file's own (hparams["noised"] is set: the models other files cache are left as they are)."""
    from matinvent_amd import predictor as PR
    m = PR.PropertyPredictor([f"p{k}" for k in range(P)], hidden_dim=H, num_layers=L, time_dim=TD, num_freqs=F, ln=True, device="cuda", seed=seed)
    gen = torch.Generator().manual_seed(seed + 100)
    for k, w in m.trunk.views().items():
        if "layer_norm" in k:
            w.add_((0.1 * torch.randn(w.shape, generator=gen)).cuda())
    m.mark_dirty()
    m.hparams["noised"] = PR.noised_spec(_diffusion())
    return m


def _params(m):
    return {"decoder." + k: v.detach().cpu() for k, v in m.state_dict().items()}


def _hp(H):
    return O.CSPNetHParams(hidden_dim=H, num_layers=L, num_freqs=F)


@functools.lru_cache(maxsize=None)
def _case(name):
    """A model, a noisy state, times and d_out, and the float32 / float64 autograd references: computed once, shared, left unchanged."""
    from matinvent_amd import predictor as PR
    if name == "g15":
        raise RuntimeError("the g15 case needs the golden fixture: _g15_case(golden)")
    H, P, na, seed = dict(loop=(64, 3, LOOP_NA, 51), grid=(64, 1, GRID_NA, 52), big=(512, 3, BIG_NA, 53))[name]
    m = _model(H, P)
    fs = SR.build_set(na, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    times = torch.randint(0, T + 1, (len(na),), generator=g)
    d_out = torch.randn(len(na), P, generator=g)
    return _finish(m, _params(m), H, fs, times, d_out, seed)


_G15 = {}


def _g15_case(golden):
    if "c" not in _G15:
        from matinvent_amd import predictor as PR
        m, P, fs = _g15(golden)
        m.hparams["noised"] = PR.noised_spec(_diffusion())
        _G15["c"] = _finish(m, P, 64, fs, torch.tensor([3, 0, 17]), torch.tensor([[0.7], [-1.3], [0.4]]), 3)
    return _G15["c"]


def _finish(m, P, H, fs, times, d_out, seed):
    types, frac, lat = _noisy_state(fs, seed)
    na = fs["num_atoms"]
    temb = O.time_embedding(times.long(), TD).float()
    ref = {dt: R.input_grad(P, _hp(H), temb, types, frac, lat, na, d_out, dt) for dt in (torch.float32, torch.float64)}
    return SimpleNamespace(m=m, P=P, H=H, fs=fs, na=na.tolist(), times=times, d_out=d_out, types=types, frac=frac, lat=lat, temb=temb, ref=ref)


def _state(c):
    return dict(atom_types=c.types.cuda(), frac_coords=c.frac.cuda(), lattices=c.lat.cuda())


def _grad_check(dev, c, k, what, tol=GRAD_TOL):
    """dev against the float32 reference at tol of max|ref|; the ratio to the float32 reference's own deviation from float64 is reported."""
    r32, r64 = c.ref[torch.float32][k].double().numpy(), c.ref[torch.float64][k].numpy()
    d = dev.detach().cpu().double().numpy().reshape(r32.shape)
    scale = max(1e-300, float(np.abs(r32).max()))
    err, own = float(np.abs(d - r32).max()) / scale, float(np.abs(r32 - r64).max()) / scale
    if os.environ.get("MI_TOL_REPORT"):
        print(f"TOL {what}: device {err:.3e} of max|ref| = {scale:.3g} (demanded {tol:.0e}); float32 reference vs float64 {own:.3e}; "
              f"ratio {err / max(own, 1e-300):.2f}; device vs float64 {float(np.abs(d - r64).max()) / scale:.3e}")
    assert np.isfinite(d).all() and err <= tol, f"{what}: device error {err:.3e} of max|ref| ({scale:.3g}) > {tol:.0e} (float32 reference's own: {own:.3e})"
    return tol * scale


def _run_case(c, what):
    from matinvent_amd import predictor as PR
    cb = c.m.make_batch(c.na)
    st = _state(c)
    keep = {k: v.clone() for k, v in st.items()}
    out, gx, gl, gt = PR.input_gradient(c.m, st, cb, c.times, d_out=c.d_out)
    bad = []
    bound_x = None
    for k, dev, nm in ((1, gx, "g_frac"), (2, gl, "g_lat"), (3, gt, "g_types")):
        try:
            b = _grad_check(dev, c, k, f"{what}: {nm}")
            bound_x = b if k == 1 else bound_x
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)
    # a one-atom crystal has no pair: exactly zero; translation invariance: the rows of a crystal sum to zero within the tensor's bound x its atoms
    off = np.concatenate([[0], np.cumsum(c.na)])
    gxc = gx.cpu()
    for b, n in enumerate(c.na):
        rows = gxc[off[b]:off[b + 1]]
        if n == 1:
            assert torch.count_nonzero(rows) == 0, f"{what}: one-atom crystal {b}"
        assert float(rows.double().sum(dim=0).abs().max()) <= bound_x * n, f"{what}: crystal {b} of {n} atoms: sum of g_frac {rows.double().sum(dim=0)}"
    # out: the taped forward against mi_scalar_forward_state's, and against the reference
    _close(out, PR.forward_state(c.m, st, cb, c.times).cpu(), FWD_TOL, f"{what}: out vs mi_scalar_forward_state")
    _close(out, c.ref[torch.float32][0], FWD_TOL, f"{what}: out vs the reference")
    # the same bits every call; the caller's arrays unchanged; g_types = NULL leaves the others as they are
    o2, gx2, gl2, gt2 = PR.input_gradient(c.m, st, cb, c.times, d_out=c.d_out)
    assert torch.equal(out, o2) and torch.equal(gx, gx2) and torch.equal(gl, gl2) and torch.equal(gt, gt2)
    o3, gx3, gl3, gt3 = PR.input_gradient(c.m, st, cb, c.times, d_out=c.d_out, types=False)
    assert gt3 is None and torch.equal(gx, gx3) and torch.equal(gl, gl3) and torch.equal(out, o3)
    assert all(torch.equal(st[k], keep[k]) for k in st)
    cb.release()


def test_the_shapes_reach_what_they_are_chosen_for():
    assert max(LOOP_NA) > 64 and min(LOOP_NA) == 1 and len(GRID_NA) == 300 and set(GRID_NA) == {1, 2, 3}
    Np, E = sum(n * (n - 1) // 2 for n in BIG_NA), sum(n * n for n in BIG_NA)
    assert Np >= 4096 and E >= 8192 and 512 % 256 == 0 and max(BIG_NA) <= 24   # the LDS-tile pair pass, whose weight gradient takes plane sets


def test_input_gradient_on_the_reference_fixture(golden):
    c = _g15_case(golden)
    assert c.times.tolist() == [3, 0, 17]
    _run_case(c, "g15 at times [3, 0, 17]")


@pytest.mark.parametrize("name", ["loop", "grid", "big"])
def test_input_gradient_vs_float32_autograd(name):
    _run_case(_case(name), name)


def test_the_data_only_form_takes_no_gradient_buffer():
    """A micro-step on the same handle after an input-gradient call gives the gradients of a handle that never ran one, bit for bit."""
    from matinvent_amd import predictor as PR
    c = _case("loop")
    yhat, have, cg = _targets(len(c.na), 3, seed=17)
    res = []
    for first in (True, False):
        cb = c.m.make_batch(c.na)
        if first:
            PR.input_gradient(c.m, _state(c), cb, c.times, d_out=c.d_out)
        grad = torch.zeros_like(c.m.flat)
        PR.train_step(c.m, _ns(c.fs), yhat=yhat, have=have, grad=grad, count_global=cg, handle=cb)
        res.append(grad)
        cb.release()
    assert torch.equal(res[0], res[1]) and res[0].any()


# ---- (2) the seed and the shift ---------------------------------------------------------------------------------------------------------

def test_guide_seed_in_three_modes_and_non_finite_rows():
    from matinvent_amd.cspnet import _ptr, _stream
    _lib, lib = _lib_()
    rng = np.random.default_rng(3)
    B, P, p, that = 300, 3, 1, 0.3
    out = rng.standard_normal((B, P)).astype(np.float32)
    out[5, p], out[17, p], out[201, p] = np.nan, np.inf, -np.inf
    out[9, 0] = np.nan   # (another column: not read)
    od = torch.from_numpy(out).cuda()
    for mode in (R.MODE_MAX, R.MODE_MIN, R.MODE_TARGET):
        d = torch.full((B, P), 7.0, device="cuda")
        _lib.check(lib.mi_guide_seed(_ptr(od), B, P, p, mode, that, _ptr(d), _stream()))
        ref = R.seed(out, p, mode, that)
        assert np.array_equal(d.cpu().numpy(), ref), mode
        assert not d[[5, 17, 201]].any() and not d[:, [0, 2]].any() and bool(d[9, p] != 0)
    for kw, text in ((dict(p=3), "property p = 3 of P = 3"), (dict(mode=3), "unknown mode"), (dict(mode=2, that=float("nan")), "target_hat is not finite")):
        a = dict(p=p, mode=0, that=0.0)
        a.update(kw)
        rc = lib.mi_guide_seed(_ptr(od), B, P, a["p"], a["mode"], a["that"], _ptr(d), _stream())
        assert rc == _lib.MI_EINVAL and text in lib.mi_last_error().decode()
    assert lib.mi_guide_seed(None, 0, 1, 0, 0, 0.0, None, _stream()) == 0


def _shift(cb, st, g, a, max_shift):
    from matinvent_amd.cspnet import _ptr, _stream
    _lib, lib = _lib_()
    rc = lib.mi_guide_shift(cb._h, _ptr(st[2]), _ptr(st[0]), _ptr(st[1]), _ptr(g[2]), _ptr(g[0]), _ptr(g[1]), a[0], a[1], a[2], max_shift, _stream())
    return rc, lib.mi_last_error().decode()


@pytest.mark.parametrize("with_types", [True, False])
@pytest.mark.parametrize("max_shift", [0.0, 0.05])
def test_guide_shift_vs_the_float64_reference(max_shift, with_types):
    na = LOOP_NA + [4, 2]
    B, N = len(na), sum(na)
    m = _model(64, 1)
    cb = m.make_batch(na)
    g = torch.Generator().manual_seed(8)
    frac, lat, types = torch.rand(N, 3, generator=g), torch.randn(B, 3, 3, generator=g), torch.randn(N, 100, generator=g)
    gx, gl, gt = torch.randn(N, 3, generator=g), torch.randn(B, 3, 3, generator=g), torch.randn(N, 100, generator=g)
    frac[0], gx[0] = torch.tensor([0.01, 0.99, 0.5]), torch.tensor([-1.0, 1.0, 0.2])   # carried across both cell boundaries
    off = np.concatenate([[0], np.cumsum(na)])
    gx[off[3] + 2, 1] = float("nan")          # crystal 3: a NaN coordinate-gradient element
    gl[5, 0, 2] = float("inf")                # crystal 5: an infinite lattice-gradient element
    if with_types:
        gt[off[6] + 1, 40] = float("nan")     # crystal 6: a NaN type-gradient element
    a = (0.07, 0.3, 0.11)
    st = (frac.cuda(), lat.cuda(), types.cuda())
    dg = (gx.cuda(), gl.cuda(), gt.cuda() if with_types else None)
    rc, msg = _shift(cb, st, dg, a, max_shift)
    assert rc == 0, msg
    r = {dt: R.shift(types, frac, lat, gt if with_types else None, gx, gl, na, *a, max_shift, dtype=dt) for dt in (np.float64, np.float32)}
    done = r[np.float64][3]
    assert done.tolist() == [True, True, True, False, True, False, not with_types]
    if max_shift > 0:   # the clamp is active for some elements and inactive for others
        v = np.abs(a[1] * gx.numpy()[np.isfinite(gx.numpy())])
        assert (v > max_shift).any() and (v < max_shift).any()
    cpu = [v.cpu() for v in st]
    circ = lambda x: x   # (coordinates are compared on the circle below)
    checks = [((cpu[1], torch.from_numpy(r[np.float64][2]), torch.from_numpy(r[np.float32][2]), "shift: lattices"), {}),
              ((cpu[0], torch.from_numpy(r[np.float64][1]), torch.from_numpy(r[np.float32][1]), "shift: coordinates"), dict(circle=True)),
              ((cpu[2], torch.from_numpy(r[np.float64][0]), torch.from_numpy(r[np.float32][0]), "shift: type rows"), {})]
    _all(checks)
    assert bool((cpu[0] >= 0).all()) and bool((cpu[0] < 1).all())
    for b in range(B):   # a crystal with a non-finite gradient element: bit-unchanged; its neighbours moved
        rows = slice(off[b], off[b + 1])
        same = torch.equal(cpu[0][rows], frac[rows]) and torch.equal(cpu[1][b], lat[b])
        assert same == (not done[b]), b
        assert torch.equal(cpu[2][rows], types[rows]) == (not done[b] or not with_types), b
    for kw, text in ((dict(a=(float("nan"), 0.1, 0.1)), "coefficient is not finite"), (dict(ms=float("inf")), "max_shift is not finite")):
        rc, msg = _shift(cb, st, dg, kw.get("a", a), kw.get("ms", 0.0))
        assert rc == _lib_()[0].MI_EINVAL and text in msg
    cb.release()


# ---- (3) the sign, end to end -------------------------------------------------------------------------------------------------------------

def test_one_shift_along_the_gradient_raises_every_crystals_output(golden):
    """MAX mode: x + a g along the device's gradient.  The step is chosen on the CPU from the references alone: along the float64
    gradient the float64 forward's own increase must exceed 100 x the float32 forward's rounding (its deviation from float64) for EVERY
    crystal -- asserted first, no crystal excluded."""
    from matinvent_amd import predictor as PR
    from matinvent_amd.cspnet import _ptr, _stream
    c = _g15_case(golden)
    m, P, hp = c.m, c.P, _hp(64)
    one = torch.ones(len(c.na), 1)
    o32, gx32, gl32, gt32 = R.input_grad(P, hp, c.temb, c.types, c.frac, c.lat, c.fs["num_atoms"], one, torch.float32)
    o64, gx64, gl64, gt64 = R.input_grad(P, hp, c.temb, c.types, c.frac, c.lat, c.fs["num_atoms"], one, torch.float64)
    rounding = float((o32.double() - o64).abs().max())
    a = None
    for cand in (1e-4, 3e-4, 1e-3, 3e-3, 1e-2):
        moved = SR.forward(P, hp, c.temb.double(), c.types.double() + cand * gt64, (c.frac.double() + cand * gx64) % 1.0, c.lat.double() + cand * gl64,
                           c.fs["num_atoms"], torch.float64)[0]
        if bool(((moved - o64) > 100 * rounding).all()):
            a = cand
            break
    assert a is not None, "no step under which the float64 reference's increase exceeds 100 x the float32 rounding for every crystal"
    cb = m.make_batch(c.na)
    st = _state(c)
    before = PR.forward_state(m, st, cb, c.times).clone()
    out, gx, gl, gt = PR.input_gradient(m, st, cb, c.times, task="y", mode="max")
    _lib, lib = _lib_()
    _lib.check(lib.mi_guide_shift(cb._h, _ptr(st["atom_types"]), _ptr(st["frac_coords"]), _ptr(st["lattices"]), _ptr(gt), _ptr(gx), _ptr(gl), a, a, a, 0.0, _stream()))
    after = PR.forward_state(m, st, cb, c.times)
    assert bool((after > before).all()), (before.flatten().tolist(), after.flatten().tolist())
    cb.release()


# ---- device-side refusals ---------------------------------------------------------------------------------------------------------------

def test_input_gradient_refusals_by_code_and_text():
    from matinvent_amd import predictor as PR
    from matinvent_amd.cspnet import _ptr, _stream
    _lib, lib = _lib_()
    c = _case("loop")
    m = c.m
    st = _state(c)
    cb = m.make_batch(c.na)
    B, N = len(c.na), sum(c.na)
    out, gx, gl = torch.full((B, 3), 7.0, device="cuda"), torch.full((N, 3), 7.0, device="cuda"), torch.full((B, 9), 7.0, device="cuda")
    d_out = c.d_out.cuda()
    m.trunk.sync()
    _, W, bias = m.head_slices()

    def call(net=m.trunk._h, h=cb, P=3, d=d_out):
        rc = lib.mi_scalar_input_grad(net, h._h, _ptr(st["atom_types"]), _ptr(st["frac_coords"]), _ptr(st["lattices"]), _ptr(m.time_freqs), None, 3,
                                      _ptr(W), _ptr(bias), P, _ptr(d), _ptr(out), None, _ptr(gx), _ptr(gl), _stream())
        return rc, lib.mi_last_error().decode()

    def refused(rc_msg, text):
        assert rc_msg[0] == _lib.MI_EINVAL and text in rc_msg[1] and "mi_scalar_input_grad" in rc_msg[1], rc_msg

    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    _lib.check(lib.mi_batch_set_time_map(cb._h, ip(np.array([0, 1, 2], np.int32)), 3))
    refused(call(), "time map")
    _lib.check(lib.mi_batch_set_time_map(cb._h, None, 0))
    _lib.check(lib.mi_batch_set_wgrad_window(m.trunk._h, cb._h, 2))
    refused(call(), "open weight-gradient window")
    _lib.check(lib.mi_batch_set_wgrad_window(m.trunk._h, cb._h, 0))
    refused(call(P=0), "at least 1")
    refused(call(d=None), "null argument")
    knn = PR.PropertyPredictor(["a", "b", "c"], hidden_dim=64, num_layers=L, time_dim=TD, num_freqs=F, ln=True, edge_style="knn", device="cuda", seed=2)
    kb = knn.make_batch([2, 3])   # (refused before anything is read: the handle's own counts do not matter)
    knn.trunk.sync()
    refused(call(net=knn.trunk._h, h=kb), "knn-style handle")
    kb.release()
    from matinvent_amd.pool import HandlePool
    pool = HandlePool()
    pb = m.make_batch(c.na, pool=pool)
    refused(call(h=pb), "pooled batch handle")
    pb.release()
    pool.close()
    from matinvent_amd.cspnet import CSPNet
    latent = CSPNet(hidden_dim=64, num_layers=L, num_freqs=F, latent_dim=TD + 16, ln=True, smooth=True, pred_type=True, device="cuda")
    _lib.check(lib.mi_net_set_latent(latent._h, 1, 8))
    latent.sync()
    cl = latent.make_batch(c.na)
    refused(call(net=latent._h, h=cl), "property-conditioned embedding")
    cl.release()
    _lib.check(lib.mi_set_edge_pairs(0))
    try:
        refused(call(), "pair mode")
    finally:
        _lib.check(lib.mi_set_edge_pairs(1))
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((gx == 7).all()) and bool((gl == 7).all())   # nothing was enqueued
    rc, msg = call()
    assert rc == 0, msg
    assert bool((gx != 7).any()) and torch.isfinite(gx).all()
    cb.release()
    with pytest.raises(ValueError, match="not noised"):
        clean = PR.PropertyPredictor(["y"], hidden_dim=64, num_layers=L, time_dim=TD, num_freqs=F, ln=True, device="cuda", seed=2)
        PR.input_gradient(clean, st, cb, 0, task="y")


# ---- (4) the chain -------------------------------------------------------------------------------------------------------------------------

CHAIN_NA = [2, 5, 1]


@functools.lru_cache(maxsize=None)
def _chain():
    from matinvent_amd import predictor as PR
    mod = _diffusion()
    pred = PR.PropertyPredictor(["x", "y"], hidden_dim=64, num_layers=L, time_dim=TD, num_freqs=F, ln=True, device="cuda", seed=12)
    pred.hparams["noised"] = PR.noised_spec(mod)
    return mod, pred


def _walk(view, c, box, seed, step_lr):
    """The guided chain with public pieces: sample(init=, t_start=, t_stop=) single steps, input_gradient (forward_state, mi_guide_seed,
    mi_scalar_input_grad), mi_guide_shift."""
    from matinvent_amd import classifier as CG, predictor as PR
    S = view.beta_scheduler.timesteps
    tau = view.time_map.tolist() if view.time_map is not None else list(range(S + 1))
    na = box.num_atoms.tolist()
    tup = lambda f: (f["frac_coords"], f["lattices"], f["atom_types"])
    state = tup(view.sample(box, seed=seed, step_lr=step_lr, t_start=S, t_stop=S)[0])   # the initial draw
    ph = c.predictor.make_batch(na)
    at, outs = S, []
    for k in c.window(S):
        if k < at:
            state = tup(view.sample(box, seed=seed, step_lr=step_lr, init=state, t_start=at, t_stop=k)[0])
        out0 = PR.forward_state(c.predictor, state, ph, tau[k])
        d_out = PR.guide_seed(c.predictor, out0, c.task, c.mode, c.target)
        out, gx, gl, gt = PR.input_gradient(c.predictor, state, ph, tau[k], d_out=d_out, types=c.guide_types)
        outs.append(out[:, c.p].cpu())
        state = tuple(v.clone() for v in tup(view.sample(box, seed=seed, step_lr=step_lr, init=state, t_start=k, t_stop=k - 1)[0]))
        CG.shift(c, ph, state, (gx, gl, gt), c.coefficients(view, step_lr, k))
        at = k - 1
    if at > 0:
        state = tup(view.sample(box, seed=seed, step_lr=step_lr, init=state, t_start=at, t_stop=0)[0])
    ph.release()
    return state, torch.stack(outs)


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("frac_coords", "lattices", "atom_types"))


@pytest.mark.parametrize("steps,kw", [(None, dict(mode="max")), (6, dict(mode="target", target=0.2, guide_types=True, max_shift=0.02)),
                                      (None, dict(mode="min", start=12, stop=8, guide_types=True))])
def test_guided_chain_equals_the_schedule_walked_with_public_pieces(steps, kw):
    from matinvent_amd import classifier as CG
    from tests.gpu_util import Box
    mod, pred = _chain()
    view = mod if steps is None else mod.respaced(steps)
    c = CG.ClassifierGuidance(pred, "y", scale=50.0, **kw)
    box, step_lr = Box(CHAIN_NA), 1e-5
    final, traj, info = view.sample(box, seed=7, step_lr=step_lr, classifier=c)
    S = view.beta_scheduler.timesteps
    want = list(range(min(kw.get("start", S), S), kw.get("stop", 0), -1))
    assert info["levels"] == want and traj[0] is final and info["out"].shape == (len(want), len(CHAIN_NA))
    assert info["times"] == ([20, 17, 13, 10, 7, 3] if steps else want)
    state, outs = _walk(view, c, box, 7, step_lr)
    assert torch.equal(final["frac_coords"], state[0]) and torch.equal(final["lattices"], state[1]) and torch.equal(final["atom_types"], state[2])
    assert torch.equal(info["out"], outs) and torch.isfinite(info["out"]).all()
    f2, _, i2 = view.sample(box, seed=7, step_lr=step_lr, classifier=c)   # two runs are the same bits
    assert _same(final, f2) and torch.equal(info["out"], i2["out"])
    assert torch.isfinite(final["frac_coords"]).all() and torch.isfinite(final["lattices"]).all()
    plain, _ = view.sample(box, seed=7, step_lr=step_lr)
    assert not torch.equal(plain["lattices"], final["lattices"]) and not torch.equal(plain["frac_coords"], final["frac_coords"])   # the shift is seen


@pytest.mark.parametrize("steps", [None, 6])
def test_a_zero_scale_leaves_the_plain_chain(steps):
    from matinvent_amd import classifier as CG
    from tests.gpu_util import Box
    mod, pred = _chain()
    view = mod if steps is None else mod.respaced(steps)
    box = Box(CHAIN_NA)
    plain, _ = view.sample(box, seed=9)
    zero = CG.ClassifierGuidance(pred, "x", scale=0.0, guide_types=True)
    f0, _, i0 = view.sample(box, seed=9, classifier=zero)
    assert _same(f0, plain) and len(i0["levels"]) == view.beta_scheduler.timesteps


def test_a_window_leaves_the_steps_outside_it_the_plain_chains():
    from matinvent_amd import classifier as CG
    from tests.gpu_util import Box
    mod, pred = _chain()
    box = Box(CHAIN_NA)
    c = CG.ClassifierGuidance(pred, "y", scale=50.0, start=12, stop=8)
    tup = lambda f: (f["frac_coords"], f["lattices"], f["atom_types"])
    # down to the window's top the guided chain IS the plain chain; behind the window it is the plain chain from the guided state
    top_g, _, info = mod.sample(box, seed=5, t_stop=12, classifier=c)
    top_p, _ = mod.sample(box, seed=5, t_stop=12)
    assert info["levels"] == [] and _same(top_g, top_p)
    at8, _, i8 = mod.sample(box, seed=5, t_stop=8, classifier=c)
    assert i8["levels"] == [12, 11, 10, 9] and not torch.equal(at8["lattices"], mod.sample(box, seed=5, t_stop=8)[0]["lattices"])
    end_g, _, _ = mod.sample(box, seed=5, classifier=c)
    end_p, _ = mod.sample(box, seed=5, init=tuple(v.clone() for v in tup(at8)), t_start=8)
    assert _same(end_g, end_p)


def test_generate_returns_records():
    from matinvent_amd import classifier as CG
    from matinvent_amd.sampling import DiffCSPSampler
    mod, pred = _chain()
    c = CG.ClassifierGuidance(pred, "y", mode="target", target=0.1, scale=1.0, max_shift=0.05, start=10)
    smp = DiffCSPSampler(batch_size=3, num_batches=1)
    data, strucs = smp.generate(mod, classifier=c)
    assert len(data) == len(strucs) == 3
    assert smp.last_classifier["levels"] == list(range(10, 0, -1)) and smp.last_classifier["out"].shape == (10, 3)

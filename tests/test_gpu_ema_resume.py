"""GPU checks of the fused Adam + weight-average step (include/matinvent_hip_ema.h; matinvent_amd/csrc/ema.hip), of FusedAdam's average,
swap and checkpoint state (matinvent_amd/optim.py) and of pretrain.fit's checkpoint / resume.

The Adam half is held to the parent's two kernels EXACTLY (torch.equal against mi_adam_step / mi_adam_step_guarded run on clones); the
average is held to a float64 restatement of  ema = d_s ema + (1 - d_s) theta_new  under the project's rule: at most
4 x the deviation of the same formula evaluated in float32 with torch from that float64 value, plus one float32 ulp of max|theta|.
Everything about resume is exact.  64-wide, 2-layer network, T = 1000, sets of 6 crystals (tests/test_gpu_pretrain.py's).

Measured on an MI355X (error / bound of the average, the largest over the sizes, step counts and decays of each case): aligned 0.48
(unguarded) and 0.21 (guarded), offset by one element 0.24 and 0.22; the step behind a skipped one 0.17.

(1) the kernel at its sizes  (2) the guard  (3) the optimizer and its state_dict  (4) the swap  (5) bit-exact resume  (6) the average
does not perturb training  (7) through the drop-in."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from matinvent_amd import _lib
from tests.gpu_util import make_module
from tests.test_gpu_pretrain import ROOT, SEED, T, _fit_set, _params, _sigmas_norm

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 3, 4, 5, 1023, 1024, 1025, 1028, 2049]   # one block covers 1024 elements in the 16-byte form
B1, B2, EPS, LR, GSCALE, MAX_NORM = 0.9, 0.999, 1e-8, 1e-3, 0.5, 1.0
ULP = 2.0 ** -23


def _ulp_of(x):
    """One float32 ulp at magnitude x (x > 0)."""
    return float(2.0 ** (np.floor(np.log2(x)) - 23)) if x > 0 else 0.0


def _decay(decay, warmup, s):
    from matinvent_amd.optim import ema_decay_at
    return ema_decay_at(decay, warmup, s)


class _Ema64:
    """The float64 restatement and its float32 evaluation with torch, advanced together from the device's own theta_new."""

    def __init__(self, ema0):
        self.e64, self.e32 = ema0.double().cpu(), ema0.float().cpu().clone()

    def step(self, theta_new, d):
        th = theta_new.detach().cpu()
        self.e64 = d * self.e64 + (1.0 - d) * th.double()
        d32 = torch.tensor(d, dtype=torch.float32)
        self.e32 = d32 * self.e32 + (torch.tensor(1.0, dtype=torch.float32) - d32) * th

    def ratio(self, ema_dev, theta):
        """(error of the device's average) / (4 x the float32 evaluation's deviation + one ulp of max|theta|); 0 for an empty vector."""
        if ema_dev.numel() == 0:
            return 0.0
        err = float((ema_dev.detach().cpu().double() - self.e64).abs().max())
        bound = 4.0 * float((self.e32.double() - self.e64).abs().max()) + _ulp_of(float(theta.detach().abs().max()))
        return err / bound


def _buffers(n, off, seed):
    """theta, exp_avg, exp_avg_sq, ema and `steps` gradients of n elements as views `off` elements into their allocations (off = 1: not
    16-byte aligned), plus a guard element behind each that must keep its bits."""
    g = torch.Generator().manual_seed(seed)

    def view(x):
        base = torch.full((n + off + 1,), 7.25, device="cuda")
        base[off:off + n] = x.cuda()
        return base
    theta = torch.randn(n, generator=g)
    return dict(theta=view(theta), m=view(0.01 * torch.randn(n, generator=g)), v=view(1e-4 * torch.rand(n, generator=g)),
                ema=view(theta * (1 + 0.01 * torch.randn(n, generator=g))), grads=[view(torch.randn(n, generator=g)) for _ in range(5)])


def _p(base, off):
    import ctypes as C
    return C.c_void_p(base.data_ptr() + 4 * off)   # (a zero-length torch view has no pointer: the entry must still get one)


def _run_case(n, off, guarded, steps, decay, warmup):
    """Returns the error / bound ratio of the average; asserts the Adam half exactly."""
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    a = _buffers(n, off, 1000 * n + 10 * off + steps)
    ref = {k: a[k].clone() for k in ("theta", "m", "v")}
    start = a["theta"].clone()
    state = torch.zeros(16, dtype=torch.int32, device="cuda")
    work = torch.empty(max(2, lib.mi_optim_workspace_bytes(n) // 4), device="cuda")
    assert (a["theta"].data_ptr() + 4 * off) % 16 == (0 if off == 0 else 4)
    r64 = _Ema64(a["ema"][off:off + n])
    for k in range(1, steps + 1):
        g = a["grads"][k - 1]
        if guarded:
            _lib.check(lib.mi_grad_norm(_p(g, off), n, GSCALE, MAX_NORM, 1, LR, B1, B2, _p(state, 0), _p(work, 0), s), "mi_grad_norm")
            _lib.check(lib.mi_adam_step_guarded(_p(ref["theta"], off), _p(g, off), _p(ref["m"], off), _p(ref["v"], off), n, B1, B2, EPS, GSCALE,
                                                _p(state, 0), s), "mi_adam_step_guarded")
            # (`step` and `lr` are ignored in this form: given values that would show)
            _lib.check(lib.mi_adam_step_ema(_p(a["theta"], off), _p(g, off), _p(a["m"], off), _p(a["v"], off), _p(a["ema"], off), n, 77, 123.0, B1, B2,
                                            EPS, GSCALE, decay, int(warmup), _p(state, 0), s), "mi_adam_step_ema")
        else:
            _lib.check(lib.mi_adam_step(_p(ref["theta"], off), _p(g, off), _p(ref["m"], off), _p(ref["v"], off), n, k, LR, B1, B2, EPS, GSCALE, s),
                       "mi_adam_step")
            _lib.check(lib.mi_adam_step_ema(_p(a["theta"], off), _p(g, off), _p(a["m"], off), _p(a["v"], off), _p(a["ema"], off), n, k, LR, B1, B2,
                                            EPS, GSCALE, decay, int(warmup), None, s), "mi_adam_step_ema")
        torch.cuda.synchronize()
        r64.step(a["theta"][off:off + n], _decay(decay, warmup, k))
    what = f"n = {n}, offset {off}, guarded {guarded}, {steps} step(s)"
    for k in ("theta", "m", "v"):
        assert torch.equal(a[k], ref[k]), f"{what}: {k} differs from the parent's kernel"   # (guard elements and prefix included)
    if n:
        assert bool(torch.isfinite(a["theta"]).all()) and bool((a["theta"][off:off + n] != start[off:off + n]).any())
    assert float(a["ema"][off + n]) == 7.25 and (off == 0 or float(a["ema"][0]) == 7.25), f"{what}: the average was written out of bounds"
    if guarded:
        assert int(state[4]) == steps and int(state[3]) == 1
    return r64.ratio(a["ema"][off:off + n], a["theta"][off:off + n])


@pytest.mark.parametrize("guarded", [False, True], ids=["unguarded", "guarded"])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset-1"])
def test_kernel_at_the_sizes_it_can_go_wrong(off, guarded):
    """Every size x 1 and 5 steps x (decay 0.999 with warm-up, decay 0.9 without): theta and both moments torch.equal to the parent's
    kernel on clones, the average within the bound of this file's docstring."""
    worst = 0.0
    for n in SIZES:
        for steps in (1, 5):
            for decay, warmup in ((0.999, True), (0.9, False)):
                r = _run_case(n, off, guarded, steps, decay, warmup)
                worst = max(worst, r)
                assert r <= 1.0, f"n = {n}, offset {off}, guarded {guarded}, {steps} steps, decay {decay}: error / bound = {r:.3f}"
    print(f"\nema error / bound, offset {off}, guarded {guarded}: worst {worst:.3f}")


# ---- (2) the guard --------------------------------------------------------------------------------------------------------------------

def _flat(n, seed=0):
    p = torch.nn.Parameter(torch.randn(n, generator=torch.Generator().manual_seed(seed)).cuda())
    p.grad = torch.zeros_like(p)
    return p


def _grads(n, k, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g).cuda() for _ in range(k)]


def _bits(x):
    return x.detach().view(torch.int32)


def test_a_skipped_step_moves_neither_the_average_nor_its_warm_up():
    from matinvent_amd.optim import FusedAdam
    n = 2049
    p, gs = _flat(n), _grads(n, 3)
    opt = FusedAdam([p], lr=1e-2, skip_nonfinite=True, ema_decay=0.999, ema_warmup=True)
    p.grad.copy_(gs[0])
    opt.step()
    torch.cuda.synchronize()
    r64 = _Ema64(opt.ema)   # (the float64 loop starts from the device's average after step 1 ...)
    before = [x.detach().clone() for x in (p, opt.ema, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])]
    bad = gs[1].clone()
    bad[1030] = float("inf")
    p.grad.copy_(bad)
    opt.step()
    torch.cuda.synchronize()
    after = (p, opt.ema, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(after, before)), "a skipped step wrote something"
    assert int(opt._opt_state[4]) == 1 and opt.state[p]["step"] == 2
    p.grad.copy_(gs[2])
    opt.step()
    torch.cuda.synchronize()
    assert int(opt._opt_state[4]) == 2
    r64.step(p, _decay(0.999, True, 2))   # (... and skips with it: the third attempted step is the second applied one, d = 3 / 12)
    r = r64.ratio(opt.ema, p)
    print(f"\nema error / bound behind a skipped step: {r:.3f}")
    assert r <= 1.0, r
    # the decay of the ATTEMPTED count (4 / 13) would lie far outside
    wrong = _decay(0.999, True, 3) * before[1].double() + (1 - _decay(0.999, True, 3)) * p.detach().double()
    assert float((wrong - opt.ema.double()).abs().max()) > 64 * ULP * float(p.detach().abs().max())


@pytest.mark.parametrize("clip", [None, 1.0], ids=["plain", "clipping"])
def test_without_skip_nonfinite_the_step_is_applied_as_the_parent_applies_it(clip):
    from matinvent_amd.optim import FusedAdam
    n = 1028
    gs = _grads(n, 2)
    gs[1][5] = float("inf")
    p, q = _flat(n), _flat(n)
    a, b = FusedAdam([p], lr=LR, max_grad_norm=clip, ema_decay=0.9), FusedAdam([q], lr=LR, max_grad_norm=clip)
    for g in gs:
        p.grad.copy_(g)
        q.grad.copy_(g)
        a.step()
        b.step()
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(q).all())
    for x, y in ((p, q), (a.state[p]["exp_avg"], b.state[q]["exp_avg"]), (a.state[p]["exp_avg_sq"], b.state[q]["exp_avg_sq"])):
        # NaN where the parent has NaN (a NaN's sign and payload carry no meaning and follow the operand order of an fma), its bits elsewhere
        nan = torch.isnan(y.detach())
        assert torch.equal(torch.isnan(x.detach()), nan) and torch.equal(_bits(x)[~nan], _bits(y)[~nan])
    assert not bool(torch.isfinite(a.ema).all())   # (the average follows the weights, as documented: clipping alone does not guard)


# ---- (3) the optimizer ------------------------------------------------------------------------------------------------------------------

def test_the_average_does_not_change_the_weights():
    from matinvent_amd.optim import FusedAdam
    n = 2049
    p, q, gs = _flat(n), _flat(n), _grads(n, 4)
    a, b = FusedAdam([p], lr=LR, ema_decay=0.9, ema_warmup=True), FusedAdam([q], lr=LR)
    start = p.detach().clone()
    for k, g in enumerate(gs):
        p.grad.copy_(g)
        q.grad.copy_(g)
        a.step()
        b.step()
        if k == 0:   # the average started as theta BEFORE the first update: d_1 = 2 / 11
            want = _decay(0.9, True, 1) * start.double() + (1 - _decay(0.9, True, 1)) * p.detach().double()
            assert float((a.ema.double() - want).abs().max()) <= 4 * ULP * float(start.abs().max())
    assert torch.equal(p, q) and torch.equal(a.state[p]["exp_avg"], b.state[q]["exp_avg"]) and not torch.equal(a.ema, p)
    assert b.ema is None
    with pytest.raises(RuntimeError, match="ema_decay"):
        with b.ema_weights():
            pass
    with pytest.raises(ValueError, match="ONE flat"):
        FusedAdam([_flat(4), _flat(4)], ema_decay=0.9)
    with pytest.raises(ValueError, match="ema"):
        FusedAdam([_flat(4)], ema_decay=1.0)


@pytest.mark.parametrize("guard", [{}, dict(max_grad_norm=1.0, skip_nonfinite=True)], ids=["unguarded", "guarded"])
def test_state_dict_round_trip_continues_the_same_run(guard, tmp_path):
    """2 steps, state_dict through torch.save / torch.load on the host, a fresh optimizer on a fresh parameter, 2 more steps: theta, both
    moments, the average and adam_steps equal 4 straight steps."""
    from matinvent_amd.optim import FusedAdam
    n = 2049
    gs = _grads(n, 4)
    kw = dict(lr=LR, ema_decay=0.9, ema_warmup=True, **guard)
    p = _flat(n)
    straight = FusedAdam([p], **kw)
    for g in gs:
        p.grad.copy_(g)
        straight.step()
    q = _flat(n)
    first = FusedAdam([q], **kw)
    for g in gs[:2]:
        q.grad.copy_(g)
        first.step()
    torch.save(dict(theta=q.detach().cpu(), opt=first.state_dict()), str(tmp_path / "opt.pt"))
    saved = torch.load(str(tmp_path / "opt.pt"), map_location="cpu", weights_only=False)
    r = _flat(n, seed=5)
    r.data.copy_(saved["theta"])
    second = FusedAdam([r], **kw)
    second.load_state_dict(saved["opt"])
    for g in gs[2:]:
        r.grad.copy_(g)
        second.step()
    torch.cuda.synchronize()
    assert torch.equal(r, p) and torch.equal(second.ema, straight.ema) and not torch.equal(second.ema, r)
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(second.state[r][k], straight.state[p][k]), k
    assert second.state[r]["step"] == 4
    if guard:
        assert int(second._opt_state[4]) == int(straight._opt_state[4]) == 4 and torch.equal(second._opt_state, straight._opt_state)
    # the refusals: other options, another length
    for other in (dict(kw, ema_decay=0.99), dict(kw, ema_warmup=False), {k: v for k, v in kw.items() if not k.startswith("ema")},
                  dict(kw, max_grad_norm=2.0), dict(kw, skip_nonfinite=not kw.get("skip_nonfinite", False))):
        with pytest.raises(ValueError, match="option"):
            FusedAdam([_flat(n)], **other).load_state_dict(saved["opt"])
    with pytest.raises(ValueError, match="numel"):
        FusedAdam([_flat(n + 1)], **kw).load_state_dict(saved["opt"])


# ---- (4) the swap -------------------------------------------------------------------------------------------------------------------------

def _module():
    return make_module(64, 2, 8, T, _params(), sigmas_norm=_sigmas_norm())


def _forward(m, na=(4, 2, 6, 3)):
    g = torch.Generator().manual_seed(3)
    B, N = len(na), sum(na)
    with torch.no_grad():
        out = m.decoder(torch.randn(B, m.decoder.latent_dim, generator=g), torch.rand(N, 100, generator=g), torch.rand(N, 3, generator=g),
                        torch.eye(3).expand(B, 3, 3) * 5 + 0.1 * torch.randn(B, 3, 3, generator=g), torch.tensor(na))
    torch.cuda.synchronize()
    return [o.clone() for o in out]


def test_inside_ema_weights_the_network_is_the_average_and_outside_it_is_itself():
    from matinvent_amd.optim import FusedAdam
    m = _module()
    theta = m.decoder.theta
    opt = FusedAdam([theta], lr=1e-2, ema_decay=0.9, ema_warmup=False)
    for g in _grads(theta.numel(), 3):
        theta.grad = g
        opt.step()
    before, raw, avg = _forward(m), theta.detach().clone(), opt.ema.clone()
    assert float((raw - avg).abs().max()) > 1e-3
    with opt.ema_weights(m.decoder):
        assert torch.equal(theta, avg) and torch.equal(opt.ema, raw)
        inside = _forward(m)
        sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}   # (what save_model writes)
        with pytest.raises(RuntimeError, match="ema_weights"):
            opt.step()
        with pytest.raises(RuntimeError, match="re-entrant"):
            with opt.ema_weights(m.decoder):
                pass
    assert torch.equal(theta, raw) and torch.equal(opt.ema, avg)
    after = _forward(m)
    m2 = _module()
    m2.load_state_dict(sd, strict=False)
    assert torch.equal(m2.decoder.theta, avg)
    from_avg = _forward(m2)
    for k in range(3):
        assert torch.equal(inside[k], from_avg[k]), f"output {k} inside the context is not the average's"
        assert torch.equal(after[k], before[k]), f"output {k} after the context: a stale packed copy"
        assert not torch.equal(inside[k], before[k])
    opt.step()   # (usable again)


# ---- (5) bit-exact resume -----------------------------------------------------------------------------------------------------------------

def _sets():
    return _fit_set()[1], _fit_set(seed=12)[1][:4]


def _assert_same_state(a, b, what):
    """Two training_state dicts, field by field, tensors bit for bit."""
    assert set(a) == set(b)
    assert torch.equal(a["theta"], b["theta"]), f"{what}: theta"
    oa, ob = a["optimizer"], b["optimizer"]
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(oa["state"][0][k], ob["state"][0][k]), f"{what}: {k}"
    assert oa["state"][0]["step"] == ob["state"][0]["step"] and oa["param_groups"] == ob["param_groups"], what
    fa, fb = oa["fused"], ob["fused"]
    assert fa["options"] == fb["options"] and fa["numel"] == fb["numel"]
    for k in ("ema", "opt_state"):
        assert (fa[k] is None) == (fb[k] is None) and (fa[k] is None or torch.equal(fa[k], fb[k])), f"{what}: {k}"
    assert a["plateau"] == b["plateau"] and a["noise_calls"] == b["noise_calls"] and a["epoch"] == b["epoch"], what
    assert a["history"] == b["history"] and a["meta"] == b["meta"], what


FULL = dict(lr=1e-3, batch_size=4, accum_steps=3, max_grad_norm=0.5, skip_nonfinite_steps=True, lr_plateau={"patience": 0, "factor": 0.5}, ema=0.9,
            handle_pool=True)
BARE = dict(lr=1e-3, batch_size=4)


@pytest.mark.parametrize("name", ["every-option", "no-option"])
def test_fit_resumed_from_a_saved_state_is_the_same_run_bit_for_bit(name, tmp_path, monkeypatch):
    """fit for 4 epochs against fit for 2, save_training_state, a freshly constructed model, load_training_state, fit(resume=...) to 4.
    every-option: batch size 4 over 6 crystals (a partial last mini-batch), accum_steps 3, clipping that bites, the non-finite guard, a
    validation set, a plateau scheduler with patience 0, ema 0.9 (validated), a poisoned handle pool."""
    from matinvent_amd import pool, pretrain
    full = name == "every-option"
    cfg = FULL if full else BARE
    data, val = _sets()
    val = val if full else None
    monkeypatch.setattr(pretrain, "HandlePool", functools.partial(pool.HandlePool, poison=True))
    quiet = dict(seed=SEED, log=lambda *_: None)
    states = {}

    def keep(tag):
        return lambda epoch, state: states.__setitem__((tag, epoch), state)
    a = _module()
    h4 = pretrain.fit(a, data, dict(cfg, epochs=4), val_list=val, checkpoint=keep("straight"), **quiet)
    b = _module()
    h2 = pretrain.fit(b, data, dict(cfg, epochs=2), val_list=val, checkpoint=keep("first"), **quiet)
    assert h2 == h4[:2] and states[("first", 1)]["epoch"] == 2
    _assert_same_state(states[("first", 1)], states[("straight", 1)], "after 2 epochs")
    path = pretrain.save_training_state(str(tmp_path / "train_state.ckpt"), states[("first", 1)])
    del b
    c = _module()
    assert not torch.equal(c.decoder.theta, a.decoder.theta)
    h = pretrain.fit(c, data, dict(cfg, epochs=4), val_list=val, checkpoint=keep("resumed"), resume=pretrain.load_training_state(path), **quiet)
    print(f"\n{name}: " + "; ".join(", ".join(f"{k} {v:.6g}" for k, v in d.items() if k in ("train_loss", "val_loss", "lr", "grad_norm", "clipped_steps",
                                                                                             "ema_decay")) for d in h4))
    assert len(h) == 4 and h == h4 and [d["lr"] for d in h] == [d["lr"] for d in h4]
    assert torch.equal(c.decoder.theta, a.decoder.theta)
    assert sorted(e for t, e in states if t == "resumed") == [2, 3]
    _assert_same_state(states[("resumed", 3)], states[("straight", 3)], "after 4 epochs")
    if full:
        oa, oc = a.fit_optimizer, c.fit_optimizer
        th = a.decoder.theta
        assert torch.equal(oc.ema, oa.ema) and not torch.equal(oa.ema, th)
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(oc.state[c.decoder.theta][k], oa.state[th][k]), k
        # the run did what the options are there for
        assert sum(d["clipped_steps"] for d in h4) >= 1 and all(d["skipped_steps"] == 0 for d in h4)
        assert h4[2]["lr"] != h4[0]["lr"], [d["lr"] for d in h4]
        assert [d["ema_decay"] for d in h4] == [_decay(0.9, True, s) for s in (1, 2, 3, 4)]
        assert c.handle_pool_stats["mallocs"] > 0
        # a different run is refused, by name
        for key, other in (("batch_size", dict(cfg, batch_size=3)), ("accum_steps", dict(cfg, accum_steps=2)), ("ema_decay", dict(cfg, ema=0.99)),
                           ("max_grad_norm", dict(cfg, max_grad_norm=1.0)), ("lr_plateau", dict(cfg, lr_plateau=None))):
            with pytest.raises(ValueError, match=key):
                pretrain.fit(_module(), data, dict(other, epochs=4), val_list=val, resume=states[("first", 1)], **quiet)
        with pytest.raises(ValueError, match="n_train"):
            pretrain.fit(_module(), data[:5], dict(cfg, epochs=4), val_list=val, resume=states[("first", 1)], **quiet)
        with pytest.raises(ValueError, match="seed"):
            pretrain.fit(_module(), data, dict(cfg, epochs=4), val_list=val, resume=states[("first", 1)], seed=SEED + 1, log=lambda *_: None)
    else:
        assert "ema_decay" not in h4[0] and "fit_optimizer" not in a.__dict__


# ---- (6) the average does not perturb training --------------------------------------------------------------------------------------------

def test_fit_with_and_without_the_average_trains_the_same_weights():
    from matinvent_amd import pretrain
    data, _ = _sets()
    runs = []
    for ema in (None, {"decay": 0.9, "warmup": False}):
        m = _module()
        h = pretrain.fit(m, data, dict(lr=1e-3, epochs=2, batch_size=4, accum_steps=1, max_grad_norm=0.5, ema=ema), seed=SEED, log=lambda *_: None)
        runs.append((m, h))
    (m0, h0), (m1, h1) = runs
    assert torch.equal(m0.decoder.theta, m1.decoder.theta)
    assert [d["ema_decay"] for d in h1] == [_decay(0.9, False, 1)] * 2 and "ema_decay" not in h0[0]
    assert [{k: v for k, v in d.items() if k != "ema_decay"} for d in h1] == h0
    assert not torch.equal(m1.fit_optimizer.ema, m1.decoder.theta)


# ---- (7) through the drop-in ----------------------------------------------------------------------------------------------------------------

def test_pretrain_with_the_average_resumes_through_the_dropin(tmp_path):
    """pipeline=pretrain for 2 epochs with ema 0.9, again to 4 epochs from models/epoch_0001, and 4 epochs straight: the same final
    last.ckpt tensor by tensor; it holds the average, loads through load_model, and each epoch's val_loss is `evaluate` on the model
    loaded from that epoch's last.ckpt."""
    from matinvent_amd import pretrain
    from matinvent_amd.pipeline import Pretrain
    from matinvent_amd.structure import write_extxyz
    from matinvent_amd.suite import DiffCSPSuite
    data, val = _sets()
    train, valp = write_extxyz(data, str(tmp_path / "train.extxyz")), write_extxyz(val, str(tmp_path / "val.extxyz"))
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        import main as dropin_main
        tiny = ["+model.hparams.decoder.hidden_dim=64", "+model.hparams.decoder.num_layers=2", "+model.hparams.decoder.num_freqs=8",
                "+model.hparams.beta_scheduler.timesteps=20", "+model.hparams.sigma_scheduler.timesteps=20", "model.head_scale=0.1"]
        common = ["pipeline=pretrain", f"pipeline.train_path={train}", f"pipeline.val_path={valp}", "pipeline.save_freq=1", "pipeline.train_cfg.batch_size=4",
                  "pipeline.train_cfg.lr=0.001", "+pipeline.train_cfg.ema=0.9", "device=cuda:0"] + tiny

        def run(args):   # (main changes into its run directory, given relative to where it starts)
            os.chdir(tmp_path)
            return dropin_main.main(args + common)
        first = run(["expname=first", "pipeline.train_cfg.epochs=2"])
        models = tmp_path / "exp_res" / "first" / "models"
        assert (models / "epoch_0001" / Pretrain.TRAIN_STATE).exists() and (models / "epoch_0000" / Pretrain.TRAIN_STATE).exists()
        assert not [f for f in os.listdir(models / "epoch_0001") if f.endswith(".tmp")]
        resumed = run(["expname=resumed", "pipeline.train_cfg.epochs=4", f"pipeline.resume_from={models / 'epoch_0001'}"])
        straight = run(["expname=straight", "pipeline.train_cfg.epochs=4"])
        assert len(first.history) == 2 and len(resumed.history) == 4 and resumed.history == straight.history and first.history == straight.history[:2]
        ck = {k: torch.load(str(tmp_path / "exp_res" / k / "models" / "final" / "last.ckpt"), map_location="cpu", weights_only=False)
              for k in ("resumed", "straight")}
        assert ck["resumed"]["weights"] == "ema" and set(ck["resumed"]) == {"state_dict", "config", "weights"}
        assert set(ck["resumed"]["state_dict"]) == set(ck["straight"]["state_dict"])
        for k, v in ck["straight"]["state_dict"].items():
            assert torch.equal(ck["resumed"]["state_dict"][k], v), k
        assert not (tmp_path / "exp_res" / "resumed" / "models" / "epoch_0001").exists()   # (the resumed run began at epoch 2)
        # last.ckpt is the average, train_state.ckpt the raw weights; the model ends the run with its raw weights
        suite = lambda path: DiffCSPSuite("diffcsp", {"batch_size": 3, "num_batches": 1}, {"batch_size": 2}, model_path=str(path), device="cuda:0")
        final = suite(tmp_path / "exp_res" / "straight" / "models" / "final").load_model()
        assert torch.equal(final.decoder.theta, straight.model.fit_optimizer.ema) and not torch.equal(final.decoder.theta, straight.model.decoder.theta)
        st = pretrain.load_training_state(str(tmp_path / "exp_res" / "straight" / "models" / "epoch_0003" / Pretrain.TRAIN_STATE))
        assert torch.equal(st["theta"], straight.model.decoder.theta.detach().cpu()) and st["epoch"] == 4
        # the epoch's val_loss is the loss of the weights its last.ckpt holds
        vset = Pretrain.read_dataset(valp)
        for e in (0, 3):
            m = suite(tmp_path / "exp_res" / "straight" / "models" / f"epoch_{e:04d}").load_model()
            got = pretrain.evaluate(m, vset, 4, seed=0)
            assert got["loss"] == straight.history[e]["val_loss"], (e, got["loss"], straight.history[e]["val_loss"])
            raw = pretrain.load_training_state(str(tmp_path / "exp_res" / "straight" / "models" / f"epoch_{e:04d}" / Pretrain.TRAIN_STATE))["theta"]
            assert not torch.equal(raw, m.decoder.theta.detach().cpu())
    finally:
        os.chdir(cwd)
        sys.path.remove(os.path.join(ROOT, "dropin"))

"""CPU checks of classifier guidance that need no GPU (matinvent_amd.classifier, predictor.input_gradient's host side,
include/matinvent_hip_inputgrad.h): the header, its table and the build list; the reference's own consistency -- a central
finite difference in float64 against float64 autograd on g15's weights; ClassifierGuidance.from_config, the window and the step
coefficients on the full grid and on a respaced grid; every host refusal by name; the drop-in config."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from matinvent_amd import _lib, classifier as CG, config as C, predictor as PR
from oracle import diffcsp_oracle as O
from tests import input_grad_ref as R
from tests import scalar_ref as SR
from tests.header_util import ROOT, declared_symbols

EXAMPLE = os.path.join(ROOT, "dropin", "configs")


def _module(T=20):
    from matinvent_amd.diffcsp import DiffCSPModule
    return DiffCSPModule(decoder=dict(hidden_dim=64, num_layers=2, num_freqs=8, ln=True, edge_style="fc"),
                         beta_scheduler=dict(timesteps=T, scheduler_mode="cosine"),
                         sigma_scheduler=dict(timesteps=T, sigma_begin=0.005, sigma_end=0.5, sigmas_norm=torch.linspace(0.7, 1.3, T + 1)),
                         device="cpu")


def _predictor(module=None, names=("density", "gap"), **kw):
    m = PR.PropertyPredictor(list(names), hidden_dim=64, num_layers=1, time_dim=256, num_freqs=8, device="cpu", seed=1, **kw)
    if module is not None:
        m.hparams["noised"] = PR.noised_spec(module)
    return m


# ---- header, table, build list ----------------------------------------------------------------------------------------------------------

def test_header_table_and_build_list():
    from matinvent_amd.build import SOURCES
    names = sorted(declared_symbols("matinvent_hip_inputgrad.h"))
    assert names == ["mi_guide_seed", "mi_guide_shift", "mi_scalar_input_grad"]
    assert sorted(_lib.INPUT_GRAD_SIGNATURES) == names
    assert any(t is _lib.INPUT_GRAD_SIGNATURES for t in _lib.EXTENSION_SIGNATURES) and _lib.EXTENSION_SIGNATURES[-1] is not _lib.INPUT_GRAD_SIGNATURES
    assert "input_grad.hip" in SOURCES
    head = open(os.path.join(ROOT, "include", "matinvent_hip_inputgrad.h")).read()
    text = open(os.path.join(ROOT, "matinvent_amd", "csrc", "guide_shift.h")).read()
    for k, name in enumerate(("MAX", "MIN", "TARGET")):
        assert f"#define MI_GUIDE_MODE_{name} {k}" in head and f"GUIDE_MODE_{name} = {k}" in text
    assert (_lib.GUIDE_MODE_MAX, _lib.GUIDE_MODE_MIN, _lib.GUIDE_MODE_TARGET) == (R.MODE_MAX, R.MODE_MIN, R.MODE_TARGET) == (0, 1, 2)
    assert os.path.exists(os.path.join(ROOT, "scripts", "guide_host_check.cpp")) and os.path.exists(os.path.join(ROOT, "scripts", "classifier_chain_timing.py"))
    # the entries bind, and their host-only refusals answer without a GPU
    lib = _lib.load()
    assert lib.mi_guide_seed(None, 4, 2, 2, 0, 0.0, None, None) == _lib.MI_EINVAL and b"property p = 2 of P = 2" in lib.mi_last_error()
    assert lib.mi_guide_seed(None, 4, 2, 0, 2, float("nan"), None, None) == _lib.MI_EINVAL and b"target_hat" in lib.mi_last_error()
    assert lib.mi_guide_shift(None, *([None] * 6), 0.0, 0.0, 0.0, 0.0, None) == _lib.MI_EINVAL
    assert lib.mi_scalar_input_grad(*([None] * 7), 0, None, None, 1, *([None] * 6)) == _lib.MI_EINVAL


# ---- the reference's own consistency ------------------------------------------------------------------------------------------------------

def test_float64_autograd_agrees_with_a_central_finite_difference(golden):
    from tests.gpu_util import params_from_golden
    g = golden("g15_pred_scalar")
    P = params_from_golden(g)
    hp = O.CSPNetHParams(hidden_dim=64, num_layers=2, num_freqs=8)
    na = torch.from_numpy(g["num_atoms"])
    gen = torch.Generator().manual_seed(3)
    N, B = int(na.sum()), len(na)
    _, onehot, fr, lat = SR.clean_inputs(g["atom_types"], g["frac"], g["lengths"], g["angles"], torch.zeros(B), 256, torch.float64)
    types = 0.8 * onehot + 0.3 * torch.randn(N, 100, generator=gen).double()
    frac = (fr + 0.1 * torch.randn(N, 3, generator=gen).double()) % 1.0
    lat = lat + 0.2 * torch.randn(B, 3, 3, generator=gen).double()
    temb = O.time_embedding(torch.tensor([3, 0, 17]), 256).double()
    d_out = torch.tensor([[0.7], [-1.3], [0.4]], dtype=torch.float64)
    out, gx, gl, gt = R.input_grad(P, hp, temb, types, frac, lat, na, d_out, torch.float64)
    assert float(gx.abs().max()) > 1e-4 and float(gl.abs().max()) > 1e-4 and float(gt.abs().max()) > 1e-4
    rng = np.random.default_rng(5)
    picks = [("frac", (int(rng.integers(N)), int(rng.integers(3))), gx) for _ in range(4)]
    picks += [("lat", (int(rng.integers(B)), int(rng.integers(3)), int(rng.integers(3))), gl) for _ in range(4)]
    picks += [("types", (int(rng.integers(N)), int(rng.integers(100))), gt) for _ in range(4)]
    for which, index, grad in picks:
        fd = R.finite_difference(P, hp, temb, types, frac, lat, na, d_out, which, index, h=1e-5)
        ref = float(grad[index])
        # a central difference at h = 1e-5: truncation ~ h^2 |f'''| and float64 cancellation ~ 1e-16 / h: 1e-6 of the tensor's largest element is far above both
        assert abs(fd - ref) <= 1e-6 * float(grad.abs().max()) + 1e-9, (which, index, fd, ref)
    # crystals are independent: the gradient of crystal 1's own term is row 1 of the batched result
    solo = torch.zeros_like(d_out)
    solo[1] = d_out[1]
    _, gx1, gl1, _ = R.input_grad(P, hp, temb, types, frac, lat, na, solo, torch.float64)
    off = np.concatenate([[0], np.cumsum(na.numpy())])
    assert torch.equal(gl1[1], gl[1]) and torch.equal(gx1[off[1]:off[2]], gx[off[1]:off[2]]) and not gl1[0].any() and not gx1[:off[1]].any()


def test_the_reference_seed_and_shift():
    out = np.array([[0.5, 1.0], [np.nan, 2.0], [0.25, np.inf]], np.float32)
    assert np.array_equal(R.seed(out, 0, R.MODE_MAX, 0.0), [[1, 0], [0, 0], [1, 0]])
    assert np.array_equal(R.seed(out, 1, R.MODE_MIN, 0.0), [[0, -1], [0, -1], [0, 0]])
    assert np.array_equal(R.seed(out, 0, R.MODE_TARGET, 0.75), [[0.25, 0], [0, 0], [0.5, 0]])
    na = [1, 2]
    frac, lat, types = np.array([[0.9, 0.1, 0.5]] * 3), np.zeros((2, 3, 3)), np.zeros((3, 100))
    gx, gl = np.array([[1.0, -1.0, 0.0]] * 3), np.ones((2, 3, 3))
    gl[1, 0, 0] = np.nan
    t, x, l, done = R.shift(types, frac, lat, None, gx, gl, na, 0.0, 0.2, 0.5, 0.15)
    assert done.tolist() == [True, False] and np.allclose(x[0], [0.05, 0.95, 0.5]) and np.array_equal(x[1:], frac[1:])
    assert np.allclose(l[0], 0.15) and not l[1].any() and not t.any()


# ---- ClassifierGuidance: from_config, the window, the coefficients --------------------------------------------------------------------------

def test_window_and_coefficients_on_the_full_and_a_respaced_grid(tmp_path):
    m = _module(20)
    p = _predictor(m)
    c = CG.ClassifierGuidance(p, "gap", scale=2.0)
    assert c.p == 1 and c.window(20) == list(range(20, 0, -1)) and c.window(20, 15) == [20, 19, 18, 17, 16] and c.window(6) == [6, 5, 4, 3, 2, 1]
    w = CG.ClassifierGuidance(p, "gap", scale=2.0, start=12, stop=8)
    assert w.window(20) == [12, 11, 10, 9] and w.window(10) == [10, 9] and w.window(20, 10) == [12, 11] and w.window(5) == []
    step_lr = 1e-5
    for view in (m, m.respaced(6)):
        tab = view._coefficients(step_lr)
        S = view.beta_scheduler.timesteps
        sig2 = view.beta_scheduler.sigmas.cpu().float() ** 2
        for t in (1, S // 2, S):
            a_t, a_x, a_l = c.coefficients(view, step_lr, t)
            assert a_t == 0.0   # the type rows are left alone
            assert abs(a_l - 2.0 * float(sig2[t])) <= 1e-6 * abs(a_l) and a_l == float(np.float32(2.0) * tab[t, 10].numpy())
            sx = view.sigma_scheduler.sigmas.cpu().double()
            want = 2.0 * (step_lr * float(sx[t] / view.sigma_scheduler.sigma_begin) ** 2 + float(sx[t] ** 2 - sx[t - 1] ** 2))
            assert abs(a_x - want) <= 1e-5 * abs(want) and a_x == float(np.float32(2.0) * (tab[t, 4] + tab[t, 6]).numpy())
        g = CG.ClassifierGuidance(p, "gap", scale=2.0, guide_types=True)
        assert g.coefficients(view, step_lr, S)[0] == g.coefficients(view, step_lr, S)[2] > 0
    v = m.respaced(6)
    tau = v.time_map.tolist()
    assert [tau[k] for k in c.window(v.beta_scheduler.timesteps)] == [20, 17, 13, 10, 7, 3]   # the predictor's trained times of a view's steps
    # from_config
    d = PR.save_predictor(p, str(tmp_path / "noised"))
    f = CG.ClassifierGuidance.from_config({"model_path": d, "task": "gap", "mode": "target", "target": 1.5, "scale": 0.5, "max_shift": 0.1, "start": 10,
                                           "stop": 2, "guide_types": True}, device="cpu")
    assert (f.mode, f.target, f.scale, f.max_shift, f.start, f.stop, f.guide_types) == ("target", 1.5, 0.5, 0.1, 10, 2, True) and f.predictor.noised["T"] == 20
    assert CG.ClassifierGuidance.from_config(f) is f and CG.ClassifierGuidance.from_config(None) is None
    with pytest.raises(ValueError, match="model_path"):
        CG.ClassifierGuidance.from_config({"task": "gap"})
    with pytest.raises(ValueError, match="unknown keys"):
        CG.ClassifierGuidance.from_config({"model_path": d, "task": "gap", "particles": 4})


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------

def test_classifier_guidance_refuses_by_name():
    m = _module(20)
    clean, p = _predictor(), _predictor(m)
    with pytest.raises(ValueError, match="not noised"):
        CG.ClassifierGuidance(clean, "gap")
    with pytest.raises(ValueError, match="knn-style"):
        CG.ClassifierGuidance(_predictor(m, edge_style="knn"), "gap")
    for kw, match in ((dict(task="volume"), "not a property"), (dict(task="gap", mode="up"), "mode"), (dict(task="gap", mode="target"), "target"),
                      (dict(task="gap", target=1.0), "target"), (dict(task="gap", mode="target", target=float("nan")), "not finite"),
                      (dict(task="gap", scale=float("inf")), "scale"), (dict(task="gap", max_shift=0.0), "max_shift"),
                      (dict(task="gap", max_shift=float("inf")), "max_shift"), (dict(task="gap", start=0), "start"), (dict(task="gap", stop=-1), "stop"),
                      (dict(task="gap", start=4, stop=4), "stop")):
        with pytest.raises(ValueError, match=match):
            CG.ClassifierGuidance(p, **kw)
    with pytest.raises(ValueError, match="not noised"):
        PR.input_gradient(clean, None, None, 0, task="gap")


def test_sample_refuses_by_name_before_any_device_work(tmp_path):
    from matinvent_amd import pipeline, sampling, steering as ST
    from matinvent_amd.conditioning import Condition
    from matinvent_amd.suite import DiffCSPSuite
    m = _module(20)
    p = _predictor(m)
    c = CG.ClassifierGuidance(p, "gap")
    ok = SimpleNamespace(num_atoms=torch.tensor([2, 3]))
    with pytest.raises(ValueError, match="streams"):
        m.sample(ok, classifier=c, streams=2)
    cond = Condition.composition([{"Na": 1, "Cl": 1}], 2)
    s = ST.Steering(p, "gap", particles=1, every=2)
    for kw, match in ((dict(record=True), "record"), (dict(noise={}), "noise"), (dict(condition=cond), "condition"), (dict(likelihood="free"), "likelihood"),
                      (dict(resample=(2, 3)), "resample"), (dict(guidance=object()), "guidance"), (dict(steer=s), "steer")):
        with pytest.raises(ValueError, match=f"classifier together with .*{match}"):
            m.sample(ok, classifier=c, **kw)
    with pytest.raises(ValueError, match="ClassifierGuidance"):
        m.sample(ok, classifier={"task": "gap"})
    other = CG.ClassifierGuidance(_predictor(_module(10)), "gap")
    with pytest.raises(ValueError, match="T = 10"):
        m.sample(ok, classifier=other)
    sig = CG.ClassifierGuidance(_predictor(m), "gap")
    sig.predictor.hparams["noised"]["sigma_scheduler"]["sigma_end"] = 1.0
    with pytest.raises(ValueError, match="schedule"):
        m.sample(ok, classifier=sig)
    with pytest.raises(ValueError, match="schedule"):
        m.respaced(6).sample(ok, classifier=sig)
    gone = CG.ClassifierGuidance(_predictor(m), "gap")
    gone.predictor.hparams.pop("noised")
    with pytest.raises(ValueError, match="not noised"):
        m.sample(ok, classifier=gone)
    knn = CG.ClassifierGuidance(_predictor(m), "gap")
    knn.predictor.hparams["edge_style"] = "knn"
    with pytest.raises(ValueError, match="knn-style"):
        m.sample(ok, classifier=knn)
    csp = _module(20)
    csp.keep_lattice = True
    with pytest.raises(ValueError, match="CSP mode"):
        csp.sample(ok, classifier=c)
    prop = _module(20)
    prop.condition = object()
    with pytest.raises(ValueError, match="property-conditioned prior"):
        prop.sample(ok, classifier=c)
    with pytest.raises(ValueError, match="MatterGen"):
        CG.check_call(SimpleNamespace(collate=None), c)
    # the trajectory layer and the policy-gradient loop
    with pytest.raises(ValueError, match="classifier"):
        sampling.sample_mdp(2, None, classifier=c)
    with pytest.raises(ValueError, match="classifier"):
        sampling.sample_rollout(2, None, classifier=c)
    suite = DiffCSPSuite("diffcsp", {"batch_size": 4, "num_batches": 1}, {}, device="cpu")
    with pytest.raises(ValueError, match="sample_cfg.classifier"):
        pipeline.MatInventPG(rl_epoch=1, model_suite=suite, reward=None, sample_cfg={"classifier": {"model_path": "/x", "task": "gap"}}, finetune_cfg={},
                             save_dir=str(tmp_path), save_freq=1, device="cpu")
    g = sampling.DiffCSPSampler(batch_size=2, num_batches=1)
    for kw, match in ((dict(condition=cond), "condition"), (dict(properties_to_condition_on={"gap": 1.0}), "properties_to_condition_on"),
                      (dict(world_size=2), "world_size"), (dict(steer=s), "steer")):
        with pytest.raises(ValueError, match=f"classifier together with .*{match}"):
            g.generate(m, classifier=c, **kw)
    # the pipelines' sample_cfg carries the key to the sampler
    rl = pipeline.ReinL(rl_epoch=1, model_suite=suite, reward=None, sample_cfg={"classifier": {"model_path": "/x", "task": "gap"}}, finetune_cfg={},
                        save_dir=str(tmp_path), save_freq=1, device="cpu")
    assert rl.sample_cfg.classifier.task == "gap"


def test_dropin_config_composes():
    cfg = C.resolved(C.compose(EXAMPLE, "base", ["+classifier@sample_cfg.classifier=predictor", "sample_cfg.classifier.model_path=/models/noised",
                                                  "sample_cfg.classifier.scale=0.25"]))
    c = cfg.sample_cfg.classifier
    assert c.model_path == "/models/noised" and c.scale == 0.25 and c.task == "density" and c.mode == "max" and c.stop == 0
    assert c.target is None and c.max_shift is None and c.start is None and c.guide_types is False
    plain = C.resolved(C.compose(EXAMPLE, "base", []))
    assert "classifier" not in plain.sample_cfg

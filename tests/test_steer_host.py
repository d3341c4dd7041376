"""CPU checks of predictor-steered sampling that need no GPU (matinvent_amd.steering, matinvent_amd.predictor's noise-aware additions,
include/matinvent_hip_steer.h): the header, its table and the build list; properties of the float64 reference of the
resampling plan (tests/steer_ref.py) -- offspring counts, the identity of equal weights, the telescoping of the increments along every
ancestry; Steering.replicate and the level schedule on a full and on a respaced grid; every host refusal by name; hparams["noised"]
through save and load; the drop-in config."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from matinvent_amd import _lib, config as C, predictor as PR, steering as ST
from tests import steer_ref as R
from tests.header_util import ROOT, declared_symbols

EXAMPLE = os.path.join(ROOT, "dropin", "configs")


def _module(T=20):
    from matinvent_amd.diffcsp import DiffCSPModule
    return DiffCSPModule(decoder=dict(hidden_dim=64, num_layers=2, num_freqs=8, ln=True, edge_style="fc"),
                         beta_scheduler=dict(timesteps=T, scheduler_mode="cosine"),
                         sigma_scheduler=dict(timesteps=T, sigma_begin=0.005, sigma_end=0.5, sigmas_norm=torch.linspace(0.7, 1.3, T + 1)),
                         device="cpu")


def _predictor(module=None, names=("density", "gap")):
    m = PR.PropertyPredictor(list(names), hidden_dim=64, num_layers=1, time_dim=256, num_freqs=8, device="cpu", seed=1)
    if module is not None:
        m.hparams["noised"] = PR.noised_spec(module)
    return m


# ---- header, table, build list ----------------------------------------------------------------------------------------------------------

def test_header_table_and_build_list():
    from matinvent_amd.build import SOURCES
    names = sorted(declared_symbols("matinvent_hip_steer.h"))
    assert names == ["mi_scalar_forward_state", "mi_scalar_micro_step_noised", "mi_steer_resample"] and len(names) == 3
    assert sorted(_lib.STEER_SIGNATURES) == names and any(t is _lib.STEER_SIGNATURES for t in _lib.EXTENSION_SIGNATURES)
    assert "steer.hip" in SOURCES
    csrc = os.path.join(ROOT, "matinvent_amd", "csrc")
    head = open(os.path.join(ROOT, "include", "matinvent_hip_steer.h")).read()
    plan = open(os.path.join(csrc, "steer_plan.h")).read()
    common = open(os.path.join(csrc, "common.h")).read()
    assert "DRAW_STEER = 29" in common and "#define MI_STEER_DRAW 29" in head and _lib.STEER_DRAW == R.DRAW_STEER == 29
    assert "#define MI_STEER_MAX_PARTICLES 256" in head and "STEER_MAX_K = 256" in plan and _lib.STEER_MAX_PARTICLES == 256
    assert (_lib.STEER_MODE_MAX, _lib.STEER_MODE_MIN, _lib.STEER_MODE_TARGET) == (R.MODE_MAX, R.MODE_MIN, R.MODE_TARGET) == (0, 1, 2)
    assert os.path.exists(os.path.join(ROOT, "scripts", "steer_host_check.cpp"))
    # the entries bind and the host-only refusals of the resampling answer without a GPU
    lib = _lib.load()
    assert lib.mi_steer_resample(None, 2, None, 1, 0, 0, 0.0, 1.0, -1.0, 0, 0, *([None] * 11)) == _lib.MI_EINVAL


# ---- properties of the reference ----------------------------------------------------------------------------------------------------------

def _random_group(rng, K, lam):
    u = rng.standard_normal(K).astype(np.float32)
    up = rng.standard_normal(K).astype(np.float32)
    lg = (0.5 * rng.standard_normal(K)).astype(np.float32)
    return u, up, lg


@pytest.mark.parametrize("K", [1, 2, 5, 64, 256])
def test_offspring_counts_are_floor_or_ceil_of_the_expected_number(K):
    rng = np.random.default_rng(K)
    for trial in range(40):
        lam = float(rng.uniform(0, 3))
        u, up, lg = _random_group(rng, K, lam)
        if trial % 4 == 0 and K > 2:
            u[rng.integers(0, K)] = np.nan
            u[rng.integers(0, K)] = -np.inf
        r = R.plan_group(u, up, lg, lam, -1.0, np.float32(rng.uniform()))
        assert r["flags"] == R.RESAMPLED
        lw = R.logweight(lg, lam, u, up).astype(np.float64)
        w = np.where(np.isneginf(lw), 0.0, np.exp(lw - lw.max()))
        expect = K * w / w.sum()
        counts = np.bincount(r["anc"], minlength=K)
        assert counts.sum() == K and np.all(counts >= np.floor(expect - 1e-9)) and np.all(counts <= np.ceil(expect + 1e-9))
        assert np.all(counts[w == 0] == 0)
        assert np.array_equal(r["u_prev"], u[r["anc"]]) and not r["logw"].any()


@pytest.mark.parametrize("K", [1, 3, 64, 256])
def test_equal_weights_give_the_identity(K):
    for U in (0.0, 0.37, np.float32(1.0) - np.float32(2.0 ** -24)):
        r = R.plan_group(np.full(K, 0.25, np.float32), np.full(K, 0.5, np.float32), np.zeros(K, np.float32), 3.0, -1.0, np.float32(U))
        assert r["flags"] == R.RESAMPLED and np.array_equal(r["anc"], np.arange(K)) and r["safe"]
        assert abs(r["ess"] - K) < 1e-9
    dead = R.plan_group(np.full(K, np.nan, np.float32), np.full(K, 0.5, np.float32), np.full(K, 0.125, np.float32), 3.0, -1.0, np.float32(0.3))
    assert dead["flags"] == R.NO_FINITE and np.array_equal(dead["anc"], np.arange(K)) and dead["ess"] == 0.0
    assert np.array_equal(dead["u_prev"], np.full(K, 0.5, np.float32)) and np.array_equal(dead["logw"], np.full(K, 0.125, np.float32))


@pytest.mark.parametrize("ess_frac", [-1.0, 0.5])
def test_increments_telescope_to_lambda_u_last_along_every_ancestry(ess_frac):
    """acc_k collects lambda (u - u_prev) of the particle's own lineage (it follows the ancestors through every resampling): after any
    number of events acc_k = lambda u_prev_k, the last score on the lineage, and the log-weight is what has accrued since the lineage's
    last resampling."""
    rng = np.random.default_rng(11)
    K, G, lam = 8, 6, 1.7
    B = G * K
    u_prev, logw, acc, since = np.zeros(B, np.float32), np.zeros(B, np.float32), np.zeros(B), np.zeros(B)
    seen = set()
    for level in range(9, -1, -1):
        out = rng.standard_normal((B, 2)).astype(np.float32)
        u = R.score(out[:, 1], R.MODE_MIN)
        inc = lam * (u.astype(np.float64) - u_prev)
        acc, since = acc + inc, since + inc
        U = R.uniforms(5, level, G, K)
        r = R.plan(out, 1, R.MODE_MIN, 0.0, lam, ess_frac, K, u_prev, logw, U)
        acc, since = acc[r["ancestors"]], since[r["ancestors"]]
        for g in range(G):
            if r["flags"][g] & R.RESAMPLED:
                since[g * K:(g + 1) * K] = 0.0
        u_prev, logw = r["u_prev"], r["logw"]
        assert np.all(r["ancestors"] // K == np.arange(B) // K)
        assert np.allclose(acc, lam * u_prev.astype(np.float64), atol=1e-5) and np.allclose(since, logw, atol=1e-5)
        seen.update(r["flags"].tolist())
    assert R.RESAMPLED in seen and (ess_frac < 0 or 0 in seen)


def test_uniforms_are_keyed_by_the_groups_first_crystal():
    from oracle import diffcsp_oracle as O
    U = R.uniforms(9, 4, 5, 3, graph_offset=7)
    assert U.dtype == np.float32 and all(U[g] == O.philox_uniform(9, 4, 29, 1, 7 + 3 * g)[0] for g in range(5))
    assert not np.array_equal(U, R.uniforms(9, 5, 5, 3, graph_offset=7))


# ---- Steering: replicate, the level schedule ------------------------------------------------------------------------------------------------

def test_replicate_and_the_level_schedule():
    m = _module(20)
    p = _predictor(m)
    s = ST.Steering(p, "gap", mode="max", particles=4, scale=2.0, every=2)
    assert s.p == 1 and s.ess_frac == -1.0 and s.target_hat == 0.0
    assert s.replicate([2, 5, 1]) == [2, 2, 2, 2, 5, 5, 5, 5, 1, 1, 1, 1] and s.replicate(torch.tensor([3])) == [3, 3, 3, 3]
    assert s.check_counts(s.replicate([2, 5, 1])) == s.replicate([2, 5, 1])
    assert s.schedule(20) == list(range(18, -1, -2)) and s.schedule(6) == [4, 2, 0] and s.schedule(20, 15) == [18, 16]
    assert ST.Steering(p, "gap", every=3).schedule(20) == [17, 14, 11, 8, 5, 2] and ST.Steering(p, "gap", every=7).schedule(6) == []
    assert ST.Steering(p, "gap", levels=[3, 0, 12, 3, 25]).schedule(20) == [12, 3, 0]
    # a respaced grid: the schedule is on the view's own step indices, the predictor's times are the trained times of those indices
    v = m.respaced(6)
    tau = v.time_map.tolist()
    assert tau == [0, 3, 7, 10, 13, 17, 20] and [tau[k] for k in s.schedule(v.beta_scheduler.timesteps)] == [13, 7, 0]
    t = ST.Steering(p, "density", mode="target", target=3.0, particles=1, every=1, ess=0.5)
    p.normalizer.mean[0], p.normalizer.std[0] = 1.0, 4.0
    assert t.target_hat == 0.5 and t.ess_frac == 0.5


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------

def test_steering_refuses_by_name():
    m = _module(20)
    clean, p = _predictor(), _predictor(m)
    assert clean.noised is None and p.noised["T"] == 20
    with pytest.raises(ValueError, match="not noised"):
        ST.Steering(clean, "gap", every=2)
    for kw, match in ((dict(task="volume", every=2), "not a property"), (dict(task="gap", mode="up", every=2), "mode"),
                      (dict(task="gap", mode="target", every=2), "target"), (dict(task="gap", target=1.0, every=2), "target"),
                      (dict(task="gap", particles=0, every=2), "particles"), (dict(task="gap", particles=257, every=2), "particles"),
                      (dict(task="gap", scale=float("inf"), every=2), "scale"), (dict(task="gap"), "exactly one"),
                      (dict(task="gap", every=2, levels=[1]), "exactly one"), (dict(task="gap", every=0), "every"),
                      (dict(task="gap", levels=[]), "levels"), (dict(task="gap", every=2, ess=0.0), "ess"), (dict(task="gap", every=2, ess=1.5), "ess")):
        with pytest.raises(ValueError, match=match):
            ST.Steering(p, **kw)


def test_sample_refuses_by_name_before_any_device_work(tmp_path):
    from matinvent_amd import pipeline, sampling
    from matinvent_amd.conditioning import Condition
    from matinvent_amd.suite import DiffCSPSuite
    m = _module(20)
    p = _predictor(m)
    s = ST.Steering(p, "gap", particles=2, every=2)
    ok = SimpleNamespace(num_atoms=torch.tensor(s.replicate([2, 3])))
    with pytest.raises(ValueError, match="K-replicated"):
        m.sample(SimpleNamespace(num_atoms=torch.tensor([2, 2, 3])), steer=s)
    with pytest.raises(ValueError, match="K-replicated"):
        m.sample(SimpleNamespace(num_atoms=torch.tensor([2, 3, 3, 2])), steer=s)
    with pytest.raises(ValueError, match="streams"):
        m.sample(ok, steer=s, streams=2)
    c = Condition.composition([{"Na": 1, "Cl": 1}], 4)
    for kw, match in ((dict(record=True), "record"), (dict(noise={}), "noise"), (dict(condition=c), "condition"), (dict(likelihood="free"), "likelihood"),
                      (dict(resample=(2, 3)), "resample"), (dict(guidance=object()), "guidance")):
        with pytest.raises(ValueError, match=match):
            m.sample(ok, steer=s, **kw)
    with pytest.raises(ValueError, match="Steering"):
        m.sample(ok, steer={"task": "gap"})
    # a predictor that is not noised (it lost the entry after the Steering was built), one of another T, one of another schedule
    other = ST.Steering(_predictor(_module(10)), "gap", particles=2, every=2)
    with pytest.raises(ValueError, match="T = 10"):
        m.sample(ok, steer=other)
    sig = ST.Steering(_predictor(m), "gap", particles=2, every=2)
    sig.predictor.hparams["noised"]["sigma_scheduler"]["sigma_end"] = 1.0
    with pytest.raises(ValueError, match="schedule"):
        m.sample(ok, steer=sig)
    with pytest.raises(ValueError, match="schedule"):
        m.respaced(6).sample(ok, steer=sig)
    gone = ST.Steering(_predictor(m), "gap", particles=2, every=2)
    gone.predictor.hparams.pop("noised")
    with pytest.raises(ValueError, match="not noised"):
        m.sample(ok, steer=gone)
    # CSP mode, the MatterGen-shaped module
    csp = _module(20)
    csp.keep_lattice = True
    with pytest.raises(ValueError, match="CSP mode"):
        csp.sample(ok, steer=s)
    with pytest.raises(ValueError, match="MatterGen"):
        ST.check_call(SimpleNamespace(collate=None), s)
    with pytest.raises(ValueError, match="MatterGen"):
        PR.noised_spec(SimpleNamespace(collate=None, base=None))
    # the trajectory layer and the policy-gradient loop
    with pytest.raises(ValueError, match="steer"):
        sampling.sample_mdp(2, None, steer=s)
    with pytest.raises(ValueError, match="steer"):
        sampling.sample_rollout(2, None, steer=s)
    suite = DiffCSPSuite("diffcsp", {"batch_size": 4, "num_batches": 1}, {}, device="cpu")
    with pytest.raises(ValueError, match="sample_cfg.steer"):
        pipeline.MatInventPG(rl_epoch=1, model_suite=suite, reward=None, sample_cfg={"steer": {"model_path": "/x", "task": "gap"}}, finetune_cfg={},
                             save_dir=str(tmp_path), save_freq=1, device="cpu")
    g = sampling.DiffCSPSampler(batch_size=2, num_batches=1)
    for kw, match in ((dict(condition=c), "condition"), (dict(properties_to_condition_on={"gap": 1.0}), "properties_to_condition_on"),
                      (dict(world_size=2), "world_size")):
        with pytest.raises(ValueError, match=match):
            g.generate(m, steer=s, **kw)
    with pytest.raises(ValueError, match="model_path"):
        ST.Steering.from_config({"task": "gap"})
    # the pipelines' sample_cfg carries the key to the sampler
    rl = pipeline.ReinL(rl_epoch=1, model_suite=suite, reward=None, sample_cfg={"steer": {"model_path": "/x", "task": "gap"}}, finetune_cfg={},
                        save_dir=str(tmp_path), save_freq=1, device="cpu")
    assert rl.sample_cfg.steer.task == "gap"


def test_noised_predictor_entry_points_refuse_by_name():
    m = _module(20)
    clean, p = _predictor(), _predictor(m)
    data = [SimpleNamespace()]
    with pytest.raises(ValueError, match="not noised"):
        PR.evaluate(clean, data, 4, t=3, diffusion=m)
    with pytest.raises(ValueError, match="diffusion"):
        PR.evaluate(p, data, 4, t=3)
    with pytest.raises(ValueError, match="without t"):
        PR.evaluate(p, data, 4, diffusion=m)
    with pytest.raises(ValueError, match="outside 0..20"):
        PR.evaluate(p, data, 4, t=21, diffusion=m)
    with pytest.raises(ValueError, match="T = 20"):
        PR.require_noised(p, "here", _module(10))
    b = SimpleNamespace(num_atoms=torch.tensor([2, 3]))
    with pytest.raises(ValueError, match="0..20"):
        PR.train_step_noised(p, b, [0, 21], m, y=np.zeros((2, 2)))
    with pytest.raises(ValueError, match="3 times for 2"):
        PR.train_step_noised(p, b, [0, 1, 2], m, y=np.zeros((2, 2)))
    t = PR.draw_noised_times(4000, 20, 3, 5, 7)
    assert t.dtype == np.int32 and t.min() == 0 and t.max() == 20 and np.array_equal(t, PR.draw_noised_times(4000, 20, 3, 5, 7))
    assert not np.array_equal(t, PR.draw_noised_times(4000, 20, 3, 6, 7))
    assert PR.noised_spec(m.respaced(6)) == PR.noised_spec(m) and PR.noised_spec(m)["sigma_scheduler"]["sigma_end"] == 0.5


# ---- the model directory ------------------------------------------------------------------------------------------------------------------

def test_noised_survives_save_and_load_and_an_older_directory_loads_without_it(tmp_path):
    m = _module(20)
    p = _predictor(m)
    d = PR.save_predictor(p, str(tmp_path / "noised"))
    q = PR.load_predictor(d, device="cpu", names=["density", "gap"])
    assert q.noised == p.noised == PR.noised_spec(m) and torch.equal(q.flat.data, p.flat.data)
    PR.require_noised(q, "here", m)
    old = PR.save_predictor(_predictor(), str(tmp_path / "clean"))   # what save_predictor wrote before this change: no `noised` entry
    assert "noised" not in open(os.path.join(old, PR.HPARAMS_FILE)).read()
    r = PR.load_predictor(old, device="cpu")
    assert r.noised is None
    with pytest.raises(ValueError, match="not noised"):
        ST.Steering(r, "gap", every=2)
    s = ST.Steering.from_config({"model_path": d, "task": "gap", "mode": "min", "particles": 3, "scale": 0.5, "every": 4, "ess": None, "target": None},
                                device="cpu")
    assert s.particles == 3 and s.mode == "min" and s.every == 4 and s.predictor.noised["T"] == 20
    assert ST.Steering.from_config(s) is s and ST.Steering.from_config(None) is None


def test_dropin_config_composes():
    cfg = C.resolved(C.compose(EXAMPLE, "base", ["+steer@sample_cfg.steer=predictor", "sample_cfg.steer.model_path=/models/noised",
                                                  "sample_cfg.steer.particles=8"]))
    s = cfg.sample_cfg.steer
    assert s.model_path == "/models/noised" and s.particles == 8 and s.task == "density" and s.mode == "max" and s.every == 10
    assert s.ess is None and s.target is None and s.scale == 1.0
    plain = C.resolved(C.compose(EXAMPLE, "base", []))
    assert "steer" not in plain.sample_cfg

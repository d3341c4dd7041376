"""CPU-only checks of the property-conditioned prior's host side (matinvent_amd/guidance.py, include/matinvent_hip_guidance.h):
the header against its ctypes table and the build's sources, the frequency table, the normaliser, the host restatement of the device's
dropout draw against the oracle's Philox, config parsing, every refusal that can be raised without a device, and the latent column's
arithmetic compiled for the host under the sanitizers."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from matinvent_amd import _lib, guidance
from matinvent_amd.build import SOURCES
from oracle import diffcsp_oracle as O
from tests import guidance_ref as GR
from tests.header_util import ROOT, declared_symbols

COND = dict(properties=["density"], num_freqs=8, p_uncond=0.1)


def test_guidance_header_is_bound_in_its_own_table_and_built():
    names = declared_symbols("matinvent_hip_guidance.h")
    assert sorted(_lib.GUIDANCE_SIGNATURES) == names and len(names) == 8 and "guidance.hip" in SOURCES
    assert any(t is _lib.GUIDANCE_SIGNATURES for t in _lib.EXTENSION_SIGNATURES)
    assert not set(names) & set(_lib.SIGNATURES)
    step, cond = _lib.PRETRAIN_SIGNATURES["mi_pretrain_micro_step"], _lib.GUIDANCE_SIGNATURES["mi_pretrain_micro_step_cond"]
    assert cond[0] == step[0] and cond[1][:len(step[1]) - 1] == step[1][:-1] and len(cond[1]) == len(step[1]) + 4   # its arguments, then four, then the stream
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in names)
    src = open(os.path.join(ROOT, "matinvent_amd", "csrc", "common.h")).read()
    assert "DRAW_COND_DROP = 28" in src and guidance.DRAW_COND_DROP == GR.DRAW_COND_DROP == 28
    head = open(os.path.join(ROOT, "include", "matinvent_hip_guidance.h")).read()
    assert f"MI_GUIDANCE_MAX_FREQS {guidance.MAX_FREQS}" in head and "MI_GUIDANCE_CLAMP 8.0f" in head and guidance.CLAMP == GR.CLAMP == 8.0


def test_host_only_entries_of_the_library():
    import ctypes
    lib = _lib.load()
    h = ctypes.c_void_p()
    cfg = _lib.NetConfig(64, 2, 8, 256 + 16, 1)
    _lib.check(lib.mi_net_create(ctypes.byref(cfg), ctypes.byref(h)))
    try:
        assert lib.mi_net_latent_dim(h) == 0
        assert lib.mi_net_set_latent(h, 1, 8) == 0 and lib.mi_net_latent_dim(h) == 16
        assert lib.mi_net_set_latent(h, 17, 8) == _lib.MI_EINVAL and b"positive even" in lib.mi_last_error() and lib.mi_net_latent_dim(h) == 16
        assert lib.mi_net_set_latent(h, 1, 13) == _lib.MI_EINVAL and lib.mi_net_set_latent(h, -1, 8) == _lib.MI_EINVAL
        assert lib.mi_net_set_latent(h, 0, 0) == 0 and lib.mi_net_latent_dim(h) == 0
    finally:
        lib.mi_net_destroy(h)


def test_property_freqs():
    f = guidance.property_freqs(12)
    assert f.dtype == torch.float32 and f.shape == (12,)
    assert torch.equal(f, GR.property_freqs(12)) and float(f[0]) == float(np.float32(np.pi / 8))
    assert all(float(f[k + 1]) == 2 * float(f[k]) for k in range(11))
    assert torch.equal(guidance.property_freqs(3), f[:3]) and guidance.latent_dim(3, 8) == 48
    for bad in (0, 13):
        with pytest.raises(ValueError, match="num_freqs"):
            guidance.property_freqs(bad)


def test_normaliser_ignores_missing_values():
    items = [SimpleNamespace(properties={"a": 1.0, "b": 5.0}), SimpleNamespace(properties={"a": 3.0, "b": None}), SimpleNamespace(properties=None),
             {"a": float("nan"), "b": 5.0}, SimpleNamespace(properties={"a": 5.0})]
    nm = guidance.PropertyNormalizer(["a", "b", "c"]).fit(items)
    assert nm.mean.tolist() == [3.0, 5.0, 0.0] and nm.std[0] == np.std([1.0, 3.0, 5.0]) and nm.std[1] == 1.0 and nm.std[2] == 1.0   # sigma = 0 -> 1; nobody has c
    yhat, have = nm(items)
    assert yhat.dtype == np.float32 and have.dtype == np.int32 and yhat.shape == have.shape == (5, 3)
    assert have.tolist() == [[1, 1, 0], [1, 0, 0], [0, 0, 0], [0, 1, 0], [1, 0, 0]]
    assert np.isfinite(yhat).all() and np.all(yhat[have == 0] == 0)
    assert yhat[0, 0] == np.float32((1.0 - 3.0) / np.std([1.0, 3.0, 5.0])) and yhat[1, 0] == 0 and yhat[0, 1] == 0
    again = guidance.PropertyNormalizer(**{("names" if k == "properties" else k): v for k, v in nm.to_dict().items()})
    assert np.array_equal(again(items)[0], yhat)
    with pytest.raises(ValueError, match="distinct"):
        guidance.PropertyNormalizer(["a", "a"])


def test_host_drop_mask_is_the_oracles_philox():
    for seed, call, B, off in ((1234, 17, 5, 0), (1234, 17, 3, 2), (7, 2 ** 32 - 1, 300, 5), (2 ** 63 + 11, 3, 9, 2 ** 33)):
        u = guidance.drop_uniforms(seed, call, B, off)
        assert u.dtype == np.float32 and np.array_equal(u, np.asarray(O.philox_uniform(seed, call, 28, B, off), dtype=np.float32))
        for p in (0.1, 0.5, 1.0):
            assert np.array_equal(guidance.drop_mask(seed, call, B, p, off), GR.drop_mask(seed, call, B, p, off))
        assert guidance.drop_mask(seed, call, B, 1.0, off).all() and not guidance.drop_mask(seed, call, B, 0.0, off).any()
    # shards drop what the whole mini-batch drops
    whole = guidance.drop_mask(1234, 17, 300, 0.3)
    assert np.array_equal(np.concatenate([guidance.drop_mask(1234, 17, 100, 0.3), guidance.drop_mask(1234, 17, 200, 0.3, 100)]), whole)
    assert 60 < whole.sum() < 120


def test_config_parsing():
    assert guidance.parse_condition(None) is None
    assert guidance.parse_condition(dict(properties="density")) == dict(properties=["density"], num_freqs=8, p_uncond=0.1)
    got = guidance.parse_condition(dict(properties=["a", "b"], num_freqs=4, p_uncond=0, mean=[1, 2], std=[3, 4]))
    assert got == dict(properties=["a", "b"], num_freqs=4, p_uncond=0.0, mean=[1.0, 2.0], std=[3.0, 4.0])
    for bad, match in ((dict(properties=[]), "properties"), (dict(properties=["a", "a"]), "properties"), (dict(properties=["a"], num_freqs=13), "num_freqs"),
                       (dict(properties=["a"], p_uncond=1.5), "p_uncond"), (dict(properties=["a"], dropout=0.1), "unknown key"),
                       (dict(properties=["a"], mean=[1, 2]), "mean")):
        with pytest.raises(ValueError, match=match):
            guidance.parse_condition(bad)
    # the shipped pipeline config documents the keys, commented out
    text = open(os.path.join(ROOT, "dropin", "configs", "pipeline", "pretrain.yaml")).read()
    assert "condition" in text and "p_uncond" in text
    assert "properties_to_condition_on" in open(os.path.join(ROOT, "dropin", "README.md")).read()


def test_guidance_values():
    nm = guidance.PropertyNormalizer(["a", "b"], mean=[1.0, 0.0], std=[2.0, 1.0])
    yhat, have = guidance.Guidance({"a": 5.0}, 2.0).arrays(nm, 3)
    assert yhat.tolist() == [[2.0, 0.0]] * 3 and have.tolist() == [[1, 0]] * 3
    yhat, have = guidance.Guidance({"b": np.array([1.0, np.nan]), "a": torch.tensor([1.0, 3.0])}).arrays(nm, 2)
    assert yhat.tolist() == [[0.0, 1.0], [1.0, 0.0]] and have.tolist() == [[1, 1], [1, 0]]
    with pytest.raises(ValueError, match="not trained on"):
        guidance.Guidance({"c": 1.0}).arrays(nm, 2)
    with pytest.raises(ValueError, match="3 values for 2"):
        guidance.Guidance({"a": [1.0, 2.0, 3.0]}).arrays(nm, 2)
    for bad in ({}, None):
        with pytest.raises(ValueError, match="non-empty dict"):
            guidance.Guidance(bad)
    with pytest.raises(ValueError, match="finite"):
        guidance.Guidance({"a": 1.0}, float("nan"))


def test_every_host_refusal_names_its_caller():
    """A module with a property part is refused by name, before any device work, by everything that fills the time embedding alone."""
    from matinvent_amd import finetune, pipeline, policy, preference, pretrain, sampling
    from matinvent_amd.diffcsp import DiffCSPModule
    fake = SimpleNamespace(condition=dict(COND), base=None)
    plain = SimpleNamespace(condition=None, base=None)
    calls = {"ft_step": lambda: finetune.ft_step(fake, plain, [], [], {}), "ft_step (prior)": lambda: finetune.ft_step(plain, fake, [], [], {}),
             "pg_step": lambda: policy.pg_step(fake, None, [], {}), "dpo_step": lambda: preference.dpo_step(fake, plain, [], [], {}),
             "sample_mdp": lambda: sampling.sample_mdp(4, fake), "sample_rollout": lambda: sampling.sample_rollout(4, fake),
             "forward_logprb": lambda: DiffCSPModule.forward_logprb(fake, {})}
    for name, call in calls.items():
        with pytest.raises(ValueError, match=name.split(" ")[0] + ": a property-conditioned prior"):
            call()
    for cls in (pipeline.MatInvent, pipeline.MatInventPG, pipeline.MatInventDPO):
        p = object.__new__(cls)
        p.model_suite = SimpleNamespace(load_model=lambda: fake)
        with pytest.raises(ValueError, match=cls.__name__ + ": a property-conditioned prior"):
            p.load_model()
    # an unconditional module takes no condition anywhere
    with pytest.raises(ValueError, match="property-conditioned module"):
        pretrain.train_step(SimpleNamespace(condition=None), None, [], y=[1.0])
    with pytest.raises(ValueError, match="property-conditioned module"):
        pretrain.train_step(SimpleNamespace(condition=None), None, [], p_uncond=0.1)
    with pytest.raises(ValueError, match="no property part"):
        DiffCSPModule.sample(plain, SimpleNamespace(num_atoms=[1]), guidance=guidance.Guidance({"density": 1.0}))
    for kw, what in ((dict(record=True), "record=True"), (dict(condition=object()), "a condition"), (dict(likelihood="free"), "likelihood"),
                     (dict(resample=(2, 2)), "resample")):
        with pytest.raises(ValueError, match="guidance together with " + what):
            DiffCSPModule.sample(SimpleNamespace(condition=dict(COND), base=None, keep_lattice=False, keep_coords=False), SimpleNamespace(num_atoms=[1]),
                                 guidance=guidance.Guidance({"density": 1.0}), **kw)
    with pytest.raises(ValueError, match="CSP mode"):
        DiffCSPModule.sample(SimpleNamespace(condition=dict(COND), base=None, keep_lattice=True, keep_coords=False), SimpleNamespace(num_atoms=[1]),
                             guidance=guidance.Guidance({"density": 1.0}))
    # fit: the config and the module must agree
    for model, spec, match in ((plain, dict(COND), "not what the module was built for"), (fake, None, "no `condition`"),
                               (fake, dict(COND, num_freqs=4), "not what the module was built for"),
                               (fake, dict(COND, properties=["gap"]), "not what the module was built for")):
        with pytest.raises(ValueError, match=match):
            pretrain._fit_condition(model, [], spec)
    with pytest.raises(ValueError, match="no training crystal carries"):
        pretrain._fit_condition(fake, [SimpleNamespace(properties=None)], dict(COND))
    # the sampler's keywords
    s = sampling.DiffCSPSampler()
    with pytest.raises(ValueError, match="needs properties_to_condition_on"):
        s.generate(None, batch_size=1, num_batches=1, diffusion_guidance_factor=2.0)
    with pytest.raises(ValueError, match="together with a condition"):
        s.generate(None, batch_size=1, num_batches=1, properties_to_condition_on={"density": 1.0}, condition=[0])


def test_run_meta_refuses_a_changed_condition():
    from matinvent_amd import pretrain
    from tests.test_ema_resume_host import _meta
    a = dict(_meta(), condition=dict(properties=["density"], num_freqs=8, p_uncond=0.1))
    pretrain.check_meta(a, dict(a))
    pretrain.check_meta(_meta(), _meta())
    for other in (_meta(), dict(a, condition=dict(a["condition"], p_uncond=0.2)), dict(a, condition=dict(a["condition"], properties=["gap"]))):
        with pytest.raises(ValueError, match=r"\bcondition = "):
            pretrain.check_meta(a, other)
        with pytest.raises(ValueError, match=r"\bcondition = "):
            pretrain.check_meta(other, a)
    opt = SimpleNamespace(options=lambda: dict(max_grad_norm=None, skip_nonfinite=False, ema_decay=None, ema_warmup=False))
    model = SimpleNamespace(beta_scheduler=SimpleNamespace(timesteps=20), decoder=SimpleNamespace(theta=torch.zeros(5)))
    assert set(pretrain.run_meta(model, opt, None, 0, 4, 1, True, 6, 0, None)) == set(pretrain.META_KEYS)
    got = pretrain.run_meta(model, opt, None, 0, 4, 1, True, 6, 0, None, dict(COND))
    assert set(got) == set(pretrain.META_KEYS) | {"condition"} and got["condition"] == COND


def test_extxyz_properties_reach_the_records(tmp_path):
    from matinvent_amd.data import CrystalData
    from matinvent_amd.pipeline import Pretrain
    from matinvent_amd.structure import write_extxyz
    d = [CrystalData(torch.rand(n, 3), torch.randint(1, 90, (n,)), torch.full((1, 3), 5.0), torch.full((1, 3), 90.0)) for n in (2, 3)]
    assert d[0].properties is None
    path = write_extxyz(d, str(tmp_path / "t.extxyz"), infos=[{"density": 4.25, "tag": "abc"}, {}])
    got = Pretrain.read_dataset(path)
    assert got[0].properties == {"density": 4.25} and got[1].properties is None and got[1].num_atoms == 3


def test_latent_column_on_the_host_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "guidance_host_check")
    subprocess.run(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "scripts", "guidance_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "ok" and len(r.stdout.splitlines()) == 13, r.stdout + r.stderr
    # ... and the host formula is the float32 reference the GPU test measures the device against
    for line in r.stdout.splitlines()[:12]:
        assert float(line.split("=")[3].split()[0]) <= float(line.split("bound")[1].strip(" )"))
    assert subprocess.run([exe, "13"], stderr=subprocess.PIPE).returncode == 2

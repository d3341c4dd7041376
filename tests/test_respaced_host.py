"""CPU-only checks of the strided reverse chain's host side: the default time grid, the re-spaced schedule tables against a
float64 re-derivation, DiffCSPModule.respaced's identity and sharing, the host refusals, and the binding of the new header."""
import ctypes

import numpy as np
import pytest
import torch

from matinvent_amd import config as C
from matinvent_amd import policy
from matinvent_amd.schedules import BetaScheduler, SigmaScheduler, respaced_schedulers, respaced_times, sampler_coefficients


def _module(T=20, device="cpu"):
    from matinvent_amd.diffcsp import DiffCSPModule
    return DiffCSPModule(decoder=dict(hidden_dim=64, num_layers=2, num_freqs=8, ln=True, edge_style="fc"),
                         beta_scheduler=dict(timesteps=T, scheduler_mode="cosine"),
                         sigma_scheduler=dict(timesteps=T, sigma_begin=0.005, sigma_end=0.5, sigmas_norm=torch.linspace(0.7, 1.3, T + 1)),
                         device=device)


@pytest.mark.parametrize("T,S", [(20, 5), (20, 7), (1000, 100), (1000, 999), (20, 20)])
def test_default_grid(T, S):
    tau = respaced_times(T, S)
    assert len(tau) == S + 1 and tau[0] == 0 and tau[-1] == T
    assert all(b > a for a, b in zip(tau, tau[1:]))
    assert all(isinstance(v, int) for v in tau)
    # linspace(0, T, S + 1) rounded half up, in exact rational arithmetic
    from fractions import Fraction
    assert tau == [(Fraction(k * T, S) + Fraction(1, 2)).__floor__() for k in range(S + 1)]
    if (T, S) == (20, 5):
        assert tau == [0, 4, 8, 12, 16, 20]
    if (T, S) == (20, 7):
        assert tau == [0, 3, 6, 9, 11, 14, 17, 20] and np.diff(tau).tolist() == [3, 3, 3, 2, 3, 3, 3]
    if (T, S) == (1000, 100):
        assert tau == list(range(0, 1001, 10))
    if (T, S) == (1000, 999):
        assert sorted(set(np.diff(tau).tolist())) == [1, 2] and np.diff(tau).tolist().count(2) == 1
    if S == T:
        assert tau == list(range(T + 1))


def test_bad_grids_are_refused():
    for S in (1, 0, -3, 21):
        with pytest.raises(ValueError, match="2..T"):
            respaced_times(20, S)
    with pytest.raises(ValueError, match="integer"):
        respaced_times(20, 4.5)
    with pytest.raises(ValueError, match="exactly one"):
        respaced_times(20)
    with pytest.raises(ValueError, match="exactly one"):
        respaced_times(20, 5, times=[0, 10, 20])
    with pytest.raises(ValueError, match="strictly increasing"):
        respaced_times(20, times=[0, 8, 8, 20])
    with pytest.raises(ValueError, match="strictly increasing"):
        respaced_times(20, times=[0, 12, 8, 20])
    with pytest.raises(ValueError, match="start at 0"):
        respaced_times(20, times=[1, 8, 20])
    with pytest.raises(ValueError, match="end at T"):
        respaced_times(20, times=[0, 8, 19])
    with pytest.raises(ValueError, match="at least three"):
        respaced_times(20, times=[0, 20])
    assert respaced_times(20, times=torch.tensor([0, 7, 20])) == [0, 7, 20]


def _ulp_close(got, ref64, what):
    """got (float32) against a float64 value: within one float32 rounding of it (half an ulp of the correctly rounded result, plus the
    re-derivation's own float64 error, far below)."""
    got, ref64 = np.asarray(got, dtype=np.float32), np.asarray(ref64, dtype=np.float64)
    r32 = ref64.astype(np.float32)
    ulp = np.spacing(np.abs(r32))
    bad = np.abs(got.astype(np.float64) - ref64) > ulp
    assert not bad.any(), f"{what}: {got[bad]} vs {ref64[bad]}"


@pytest.mark.parametrize("T,S", [(20, 7), (1000, 100)])
def test_respaced_buffers_match_a_float64_rederivation(T, S):
    beta = BetaScheduler(T, "cosine")
    sn = torch.cat([torch.ones(1), torch.linspace(1.2, 0.4, T)])
    sigma = SigmaScheduler(T, 0.005, 0.5, sigmas_norm=sn)
    tau = respaced_times(T, S)
    b, s = respaced_schedulers(beta, sigma, tau)
    assert b.timesteps == s.timesteps == S and s.sigma_begin == 0.005 and s.sigma_end == 0.5
    acp = beta.alphas_cumprod.numpy().astype(np.float64)     # the stored float32 buffer, upcast
    tau = np.asarray(tau)
    al = np.ones(S + 1)
    al[1:] = acp[tau[1:]] / acp[tau[:-1]]
    be = 1.0 - al
    sg = np.zeros(S + 1)
    sg[1:] = np.sqrt(be[1:] * (1.0 - acp[tau[:-1]]) / (1.0 - acp[tau[1:]]))
    for k in ("betas", "alphas", "alphas_cumprod", "sigmas"):
        assert getattr(b, k).dtype == torch.float32 and getattr(b, k).shape == (S + 1,)
    assert np.array_equal(b.alphas_cumprod.numpy(), beta.alphas_cumprod.numpy()[tau])
    _ulp_close(b.alphas.numpy(), al, "alphas")
    _ulp_close(b.betas.numpy(), be, "betas")
    _ulp_close(b.sigmas.numpy(), sg, "sigmas")
    assert float(b.alphas[0]) == 1.0 and float(b.betas[0]) == 0.0 and float(b.sigmas[0]) == 0.0
    assert np.array_equal(s.sigmas.numpy(), sigma.sigmas.numpy()[tau])
    assert np.array_equal(s.sigmas_norm.numpy(), sigma.sigmas_norm.numpy()[tau])
    # the product of the re-spaced alphas telescopes back to the trained grid's cumulative product
    np.testing.assert_allclose(np.cumprod(b.alphas.numpy().astype(np.float64)), acp[tau], rtol=1e-6 * S)
    # sampler_coefficients runs on the pair as it stands: its adjacent sigma is sigmas[tau_{k-1}]
    coef = sampler_coefficients(b, s, 5e-6)
    assert coef.shape[0] == S + 1
    sx = sigma.sigmas.numpy().astype(np.float64)
    np.testing.assert_allclose(coef[2:, 6].numpy(), sx[tau[2:]] ** 2 - sx[tau[1:-1]] ** 2, rtol=1e-5)


def test_identity_and_sharing():
    m = _module(20)
    assert m.base is None and m.time_map is None
    assert m.respaced(20) is m
    assert m.respaced(times=list(range(21))) is m
    v = m.respaced(7)
    assert v is not m and v.base is m
    assert v.time_map.dtype == torch.int32 and v.time_map.tolist() == [0, 3, 6, 9, 11, 14, 17, 20]
    assert v.decoder is m.decoder and v.decoder.theta is m.decoder.theta
    assert v.time_embedding is m.time_embedding
    assert (v.keep_lattice, v.keep_coords) == (m.keep_lattice, m.keep_coords)
    assert (v.cost_lattice, v.cost_coord, v.cost_type) == (m.cost_lattice, m.cost_coord, m.cost_type)
    assert v.beta_scheduler.timesteps == 7 and v.sigma_scheduler.timesteps == 7
    assert m.beta_scheduler.timesteps == 20 and m.beta_scheduler.alphas.shape == (21,)
    # its own coefficient-table cache: the base's table is untouched by the view's
    cm, cv = m._coefficients(5e-6), v._coefficients(5e-6)
    assert cm.shape[0] == 21 and cv.shape[0] == 8
    assert v.__dict__["_coef_cache"] is not m.__dict__["_coef_cache"]
    assert m._coefficients(5e-6) is cm and v._coefficients(5e-6) is cv
    # one view per grid, and an explicit grid
    assert m.respaced(7) is v and m.respaced(times=v.time_map) is v
    e = m.respaced(times=[0, 1, 5, 20])
    assert e.time_map.tolist() == [0, 1, 5, 20] and e.beta_scheduler.timesteps == 3 and e.base is m
    with pytest.raises(ValueError, match="view already"):
        v.respaced(3)
    # the parameters reached through the view are the base's (one flat theta), and the base does not list its views as submodules
    assert [id(p) for p in v.parameters()] == [id(p) for p in m.parameters()]
    assert all(sub is not v for sub in m.modules())


class _FakeRollout:
    def __init__(self, T, B=3):
        self.T, self.num_graphs = T, B
        self.num_atoms = torch.tensor([2] * B)


def test_pg_step_host_refusals():
    m, other = _module(20), _module(20)
    v = m.respaced(5)
    cfg = dict(lr=1e-4, epochs=1, timesteps=2, accum_steps=1)
    rewards = np.array([0.1, 0.5, 0.9])
    with pytest.raises(ValueError, match="T = 20"):
        policy.pg_step(v, _FakeRollout(20), rewards, cfg)                    # a full-grid rollout, a strided agent
    with pytest.raises(ValueError, match="T = 5"):
        policy.pg_step(m, _FakeRollout(5), rewards, cfg)                     # and the reverse
    kl = dict(cfg, kl_coef=0.1)
    with pytest.raises(ValueError, match="time map"):
        policy.pg_step(v, _FakeRollout(5), rewards, kl, prior=other)         # prior on the trained grid
    with pytest.raises(ValueError, match="time map"):
        policy.pg_step(v, _FakeRollout(5), rewards, kl, prior=other.respaced(times=[0, 4, 8, 12, 15, 20]))   # same S, another grid
    with pytest.raises(ValueError, match="time map"):
        policy.pg_step(m, _FakeRollout(20), rewards, kl, prior=other.respaced(5))
    assert policy._same_time_map(v, other.respaced(5)) and policy._same_time_map(m, other)


def test_mattergen_suite_refuses_sample_steps(tmp_path):
    from matinvent_amd import pipeline
    from matinvent_amd.mattergen import MatterGenSampler
    from matinvent_amd.suite import DiffCSPSuite, MatterGenSuite
    suite = MatterGenSuite("mattergen", {"batch_size": 4, "num_batches": 1, "sample_steps": 10}, {}, device="cpu")
    with pytest.raises(ValueError, match="sampling_steps"):
        suite.get_sampler()
    ok = MatterGenSuite("mattergen", {"batch_size": 4, "num_batches": 1, "sample_steps": None}, {}, device="cpu")
    assert ok.get_sampler().n_steps == 1000
    with pytest.raises(ValueError, match="sampling_steps"):       # the key arriving through the pipeline's sample_cfg
        pipeline.ReinL(rl_epoch=1, model_suite=ok, reward=None, sample_cfg={"sample_steps": 10}, finetune_cfg={}, save_dir=str(tmp_path),
                       save_freq=1, device="cpu")
    with pytest.raises(ValueError, match="n_steps"):
        MatterGenSampler(batch_size=2, num_batches=1).generate(None, sample_steps=10)
    # the DiffCSP suite takes it: the pipeline reads it from the merged sample_cfg
    d = DiffCSPSuite("diffcsp", {"batch_size": 4, "num_batches": 1}, {}, device="cpu")
    rl = pipeline.ReinL(rl_epoch=1, model_suite=d, reward=None, sample_cfg={"sample_steps": 10}, finetune_cfg={}, save_dir=str(tmp_path),
                        save_freq=1, device="cpu")
    assert rl.sample_cfg.sample_steps == 10


def test_example_config_keeps_the_key_commented_out():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = C.resolved(C.compose(os.path.join(root, "dropin", "configs"), "base", ["eval_size=6", "device=cuda:0"]))
    assert "sample_steps" not in cfg.sample_cfg and "sample_steps" not in cfg.pipeline.sample_cfg
    text = open(os.path.join(root, "dropin", "configs", "base.yaml")).read()
    assert "# sample_steps:" in text


def test_stride_header_is_exported_and_bound_in_its_own_table():
    from matinvent_amd import _lib
    from matinvent_amd.build import build
    from tests.header_util import declared_symbols
    names = declared_symbols("matinvent_hip_stride.h")
    assert names == ["mi_batch_set_time_map"]
    lib = ctypes.CDLL(build(verbose=False))
    assert hasattr(lib, "mi_batch_set_time_map")
    assert sorted(_lib.STRIDE_SIGNATURES) == names and any(t is _lib.STRIDE_SIGNATURES for t in _lib.EXTENSION_SIGNATURES)
    assert not set(names) & set(_lib.SIGNATURES)
    bound = _lib.load()
    assert bound.mi_batch_set_time_map.argtypes == _lib.STRIDE_SIGNATURES["mi_batch_set_time_map"][1]
    # refused on the host, before any device work: a null handle
    assert bound.mi_batch_set_time_map(None, None, 0) == _lib.MI_EINVAL
    assert b"null handle" in bound.mi_last_error()

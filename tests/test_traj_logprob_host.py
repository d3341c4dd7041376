"""CPU-only checks of the trajectory log-probabilities (DiffCSPModule.forward_logprb, sample_mdp): the library exports and binds the
trajectory extension header, the reference-generated fixture g13 is reproduced by the oracle's restatement (what the GPU tests
compare against), and the drop-in import paths resolve."""
import ctypes
import importlib
import os
import sys

import numpy as np
import torch

from tests.header_util import ROOT, declared_symbols
from tests.traj_util import STATE_KEYS, forward_logprb, hparams_of


def test_library_exports_and_binds_exactly_the_trajectory_header():
    from matinvent_amd import _lib
    from matinvent_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    names = declared_symbols("matinvent_hip_traj.h")
    assert names == ["mi_traj_logprob", "mi_traj_logprob_backward"]
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/matinvent_hip_traj.h but not exported"
    assert sorted(_lib.TRAJ_SIGNATURES) == names
    # a table of its own: the boundary + debug table stays exactly the two other headers' declarations
    assert not set(names) & set(_lib.SIGNATURES)
    assert sorted(_lib.SIGNATURES) == sorted(declared_symbols() + declared_symbols("matinvent_hip_debug.h"))
    bound = _lib.load()
    for n in names:
        assert getattr(bound, n).argtypes == _lib.TRAJ_SIGNATURES[n][1]


def test_trajectory_entries_reject_bad_handles_without_a_gpu():
    lib = __import__("matinvent_amd._lib", fromlist=["load"]).load()
    z = [None] * 20
    assert lib.mi_traj_logprob(*z[:5], 20, *z[6:18], 1, None) == -1        # MI_EINVAL: null handles
    assert b"null handle" in lib.mi_last_error()
    assert lib.mi_traj_logprob_backward(*[None] * 9) == -1


def _g13(golden):
    g = golden("g13_forward_logprb")
    P = {k[3:]: torch.from_numpy(np.asarray(g[k])) for k in g.files if k.startswith("P__")}
    beta = {k: P[f"beta_scheduler.{k}"] for k in ("alphas", "alphas_cumprod", "sigmas")}
    sigma = {k: P[f"sigma_scheduler.{k}"] for k in ("sigmas", "sigmas_norm")}
    return g, P, beta, sigma


def _state(g, t):
    na = torch.from_numpy(g["num_atoms"])
    s = {k: torch.from_numpy(g[f"t{t}_{k}"]) for k in STATE_KEYS}
    s.update(num_atoms=na, timesteps=torch.full((len(na),), int(t), dtype=torch.long))
    return s


def _rel(a, b, tol, what):
    a, b = a.detach().numpy(), np.asarray(b)
    scale = max(1e-12, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    assert err <= tol * scale, f"{what}: max abs err {err:.3e} > {tol:.0e} * max|ref| ({scale:.3g})"


def test_g13_is_reproduced_by_the_oracle(golden):
    """The oracle's forward_logprb (cspnet_forward + the reference's formulas, tests/traj_util.py) reproduces the reference's log-probs,
    corrector predictions and accumulated parameter gradients (torch autograd through the oracle) within 1e-6 of each quantity's scale."""
    g, P, beta, sigma = _g13(golden)
    hp = hparams_of(P)
    assert (hp.hidden_dim, hp.num_layers, hp.num_freqs) == (64, 2, 8)
    freqs = torch.from_numpy(g["time_freqs"])
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items() if k.startswith("decoder.")}
    for t in g["ts"]:
        lp_l, lp_t, lp_x, (pl, px, pt) = forward_logprb(Pg, hp, beta, sigma, 0.005, _state(g, t), float(g["step_lr"]), freqs)
        for k, v in (("log_prob_l", lp_l), ("log_prob_t", lp_t), ("log_prob_x", lp_x), ("pred_l_corr", pl), ("pred_x_corr", px),
                     ("pred_t_corr", pt)):
            _rel(v, g[f"t{t}_{k}"], 1e-6, f"t={t} {k}")
        w = {k: torch.from_numpy(g[f"t{t}_w_{k}"]) for k in "ltx"}
        v = {k: torch.from_numpy(g[f"t{t}_v_{k}"]) for k in "ltx"}
        loss = (w["l"] * lp_l).sum() + (w["t"] * lp_t).sum() + (w["x"] * lp_x).sum() + (v["l"] * pl).sum() + (v["x"] * px).sum() + (v["t"] * pt).sum()
        loss.backward()
    for k, p in Pg.items():
        _rel(p.grad, g["G__" + k], 1e-6, f"grad {k}")


def test_oracle_mixed_timesteps_equal_separate_calls(golden):
    """Per-crystal timesteps (the device path's generalisation) are per-crystal: a mixed call equals the calls at each t."""
    g, P, beta, sigma = _g13(golden)
    hp = hparams_of(P)
    freqs = torch.from_numpy(g["time_freqs"])
    ts = [int(t) for t in g["ts"]]
    na = torch.from_numpy(g["num_atoms"])
    pick = {b: ts[b % len(ts)] for b in range(len(na))}
    off = [0] + torch.cumsum(na, 0).tolist()
    mixed = {}
    for k in STATE_KEYS:
        parts = [torch.from_numpy(g[f"t{pick[b]}_{k}"]) for b in range(len(na))]
        if "lattices" in k:
            mixed[k] = torch.stack([parts[b][b] for b in range(len(na))])
        else:
            mixed[k] = torch.cat([parts[b][off[b]:off[b + 1]] for b in range(len(na))])
    mixed.update(num_atoms=na, timesteps=torch.tensor([pick[b] for b in range(len(na))]))
    out = forward_logprb(P, hp, beta, sigma, 0.005, mixed, float(g["step_lr"]), freqs)
    for b in range(len(na)):
        for i, k in enumerate(("log_prob_l", "log_prob_t", "log_prob_x")):
            assert abs(float(out[i][b]) - float(g[f"t{pick[b]}_{k}"][b])) <= 1e-6 * max(1.0, abs(float(g[f"t{pick[b]}_{k}"][b]))), (b, k)


def test_dropin_import_paths():
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        sample = importlib.import_module("models.diffcsp.sample")
        diffusion = importlib.import_module("models.diffcsp.diffusion")
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
    from matinvent_amd import sampling
    assert sample.sample_mdp is sampling.sample_mdp and sample.sample_loop is sampling.sample_loop
    assert callable(diffusion.DiffCSPModule.forward_logprb)
    # the host utilities the reference module exports, against the oracle's restatement
    x, mu = torch.rand(50, 3), torch.rand(50, 3)
    assert torch.equal(diffusion.log_prob_wn(x, mu, torch.tensor(0.1)), __import__("oracle.diffcsp_oracle", fromlist=["x"]).log_prob_wn(x, mu, torch.tensor(0.1)))
    assert torch.allclose(diffusion.p_wrapped_normal(x - mu, torch.tensor(0.1)), torch.exp(diffusion.log_prob_wn(x, mu, torch.tensor(0.1))))

"""CPU checks of the property predictor: tests/scalar_ref.py against the reference-recorded fixture g15, the new header
against its ctypes table, the closed-form seeds and statistics against autograd of the stated loss, rewards.Surrogate through
Reward.scoring, the host refusals by name, and the drop-in configs."""
import os
import sys

import numpy as np
import pytest
import torch

from matinvent_amd import _lib
from matinvent_amd import config as C
from tests import scalar_ref as SR
from tests.header_util import declared_symbols
from tests.test_oracle_golden import TINY, close, params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "dropin", "configs")


def test_scalar_ref_reproduces_the_reference_fixture(golden):
    """g15: the reference's CSPNet(pred_scalar=True, smooth=True) on three crystals of [1, 7, 3] atoms.  The clean inputs are rebuilt from
    the labelled crystal; the output at the tolerance test_oracle_golden.test_cspnet_tiny holds the forward outputs to (rtol = atol = 1e-5)."""
    g = golden("g15_pred_scalar")
    assert g["num_atoms"].tolist() == [1, 7, 3] and g["scalar"].shape == (3, 1)
    P = params(g)
    assert P["decoder.scalar_out.weight"].shape == (1, 64) and P["decoder.scalar_out.bias"].shape == (1,)
    t_emb, onehot, fr, lat = SR.clean_inputs(g["atom_types"], g["frac"], g["lengths"], g["angles"], g["times"], 256, torch.float32)
    close(onehot, g["onehot"], rtol=0, atol=0)
    close(t_emb, g["t_emb"], rtol=0, atol=0)
    close(lat, g["lattices"], rtol=1e-6, atol=1e-6)
    out, gf, _ = SR.forward(P, TINY, t_emb, onehot, fr, lat, g["num_atoms"])
    close(out, g["scalar"], rtol=1e-5, atol=1e-5)
    out64, _, _ = SR.forward(P, TINY, *SR.clean_inputs(g["atom_types"], g["frac"], g["lengths"], g["angles"], g["times"], 256, torch.float64),
                             g["num_atoms"], dtype=torch.float64)
    close(out64.float(), g["scalar"], rtol=1e-5, atol=1e-5)


def test_header_table_and_build_list():
    from matinvent_amd.build import SOURCES
    names = declared_symbols("matinvent_hip_scalar.h")
    assert names == sorted(_lib.SCALAR_SIGNATURES) and len(names) == 3
    assert any(t is _lib.SCALAR_SIGNATURES for t in _lib.EXTENSION_SIGNATURES)
    assert "scalar_head.hip" in SOURCES
    src = open(os.path.join(ROOT, "include", "matinvent_hip_scalar.h")).read()
    assert f"#define MI_SCALAR_LOSS_MSE {_lib.SCALAR_LOSS_MSE}" in src and f"#define MI_SCALAR_LOSS_L1 {_lib.SCALAR_LOSS_L1}" in src


@pytest.mark.parametrize("kind", [SR.MSE, SR.L1])
def test_closed_form_seeds_and_statistics_equal_autograd(kind):
    """B = 7, P = 3: rows without any target, a property absent from this shard whose count_global is positive, missing targets that hold
    NaN; accum_steps = 3."""
    g = torch.Generator().manual_seed(3)
    B, Pn = 7, 3
    out = torch.randn(B, Pn, generator=g, dtype=torch.float64)
    yhat = torch.randn(B, Pn, generator=g, dtype=torch.float64)
    have = (torch.rand(B, Pn, generator=g) < 0.6).int()
    have[2] = 0          # a crystal whose targets are all missing
    have[:, 1] = 0       # a property nobody in the shard has ...
    have[0, 0] = have[1, 2] = 1
    yhat[have == 0] = float("nan")
    cg = have.sum(dim=0) + torch.tensor([2, 5, 0])   # ... though the whole mini-batch does
    assert int(cg[1]) == 5 and int(have[:, 1].sum()) == 0
    s = SR.seeds(out, yhat, have, cg, kind, accum=3)
    a = SR.seeds_autograd(out, yhat, have, cg, kind, accum=3)
    assert torch.isfinite(s).all() and torch.isfinite(a).all()
    np.testing.assert_allclose(s.numpy(), a.numpy(), rtol=1e-14, atol=0)
    assert torch.count_nonzero(s[have == 0]) == 0 and torch.count_nonzero(s[2]) == 0 and torch.count_nonzero(s[:, 1]) == 0
    st = SR.stats(out, yhat, have, cg, kind)
    assert st.shape == (1 + 3 * Pn,) and torch.isfinite(st).all()
    # one element at a time, in Python floats
    tot, per = 0.0, [[0.0, 0.0, 0.0] for _ in range(Pn)]
    for p in range(Pn):
        for b in range(B):
            if int(have[b, p]):
                e = float(out[b, p]) - float(yhat[b, p])
                per[p][0] += e * e
                per[p][1] += abs(e)
                per[p][2] += 1.0
        if int(cg[p]) > 0:
            tot += (per[p][0] if kind == SR.MSE else per[p][1]) / int(cg[p]) / Pn
    np.testing.assert_allclose(st.numpy(), np.array([tot] + [v for q in per for v in q]), rtol=1e-13, atol=0)
    assert st[1 + 3 * 1:4 + 3 * 1].tolist() == [0.0, 0.0, 0.0]
    assert abs(float(SR.loss(out, yhat, have, cg, kind)) - tot) <= 1e-13 * abs(tot)


class _StubPredictor:
    names = ["density", "gap"]

    def __init__(self):
        self.seen = []

    def predict(self, records, batch_size=64):
        self.seen.append((len(records), batch_size))
        out = np.array([[float(np.mean(r.species)), 10.0 * len(r.species)] for r in records])
        out[[i for i, r in enumerate(records) if 99 in r.species]] = np.nan   # a crystal the predictor cannot evaluate
        return out


def _strucs():
    from matinvent_amd.data import SimpleStructure
    sp = [[1, 3], [99, 2], [8], [4, 4, 4, 12]]
    return [SimpleStructure([4.0, 5.0, 6.0], [90.0, 90.0, 90.0], s, np.zeros((len(s), 3))) for s in sp]


def test_surrogate_through_reward_scoring(tmp_path):
    from matinvent_amd.rewards import PyMatGen, Reward, Surrogate
    stub = _StubPredictor()
    cfg = [dict(name="density_hat", calculator=Surrogate(predictor=stub, task="density", batch_size=3), target="ascending", minv=0.0, maxv=10.0),
           dict(name="gap_hat", calculator=Surrogate(predictor=stub, task="gap"), target=20.0, minv=0.0, maxv=40.0),
           dict(name="density", calculator=PyMatGen(task="density"), target="descending", minv=0.0, maxv=10.0)]
    r, props, failed = Reward(str(tmp_path / "rw"), cfg, 0.5, reduce="mean").scoring((_strucs(), None), "x")
    assert failed.tolist() == [False, True, False, False] and r[1] == 0.0
    assert props["density_hat"].tolist() == [2.0, 0.0, 8.0, 6.0]          # the records' order is kept; NaN is reported as 0 and failed
    assert props["gap_hat"].tolist() == [20.0, 0.0, 10.0, 40.0]
    assert stub.seen[0] == (4, 3) and stub.seen[1] == (4, 64)
    want0 = np.mean([0.2, 1.0, np.clip((-props["density"][0] + 10.0) / 10.0, 0, 1)])
    assert abs(r[0] - want0) <= 1e-12 and np.all(r[[0, 2, 3]] > 0)
    assert Surrogate(predictor=stub, task="gap").calc([], "x").shape == (0,)


def test_host_refusals_by_name(tmp_path, monkeypatch):
    from matinvent_amd import dist, predictor
    from matinvent_amd.rewards import Surrogate
    monkeypatch.setattr(dist, "rank_world", lambda: (0, 2))
    with pytest.raises(ValueError, match="world size 2"):
        predictor.fit_predictor(None, [], dict(lr=1e-3, epochs=1, batch_size=2))
    monkeypatch.undo()
    with pytest.raises(ValueError, match="latent"):
        predictor.PropertyPredictor(["density"], hidden_dim=64, num_layers=1, latent_dim=16)
    with pytest.raises(ValueError, match="unknown property name 'hardness'"):
        Surrogate(predictor=_StubPredictor(), task="hardness")
    with pytest.raises(ValueError, match="exactly one"):
        Surrogate(task="density")
    # a saved model: hparams.yaml names its properties, and a load that expects others is refused before any weight is read
    hp = dict(names=["density", "gap"], hidden_dim=64, num_layers=1, time_dim=256, num_freqs=8, ln=True, edge_style="fc")
    from matinvent_amd.guidance import PropertyNormalizer
    d = str(tmp_path / "model")
    predictor.write_hparams(d, hp, PropertyNormalizer(hp["names"], [1.0, 2.0], [3.0, 4.0]))
    got = predictor.read_hparams(d, names=["density", "gap"])
    assert got["names"] == hp["names"] and got["mean"] == [1.0, 2.0] and got["std"] == [3.0, 4.0] and got["hidden_dim"] == 64
    with pytest.raises(ValueError, match=r"names \['density', 'gap'\] differ from the expected names \['gap', 'density'\]"):
        predictor.load_predictor(d, names=["gap", "density"])
    with pytest.raises(ValueError, match="unknown property name 'hardness'"):
        Surrogate(model_path=d, task="hardness")
    assert Surrogate(model_path=d, task="gap").predictor is None   # (the weights are read on first use)
    with pytest.raises(ValueError, match="distinct and at least one"):
        predictor.PropertyPredictor([])
    with pytest.raises(ValueError, match="'mse' or 'l1'"):
        predictor.train_step(None, None, loss="huber")


def test_cspnet_pred_scalar_keeps_raising():
    """(the refusal stands in front of the library load: no GPU is needed)"""
    from matinvent_amd.cspnet import CSPNet
    with pytest.raises(NotImplementedError, match="DiffCSPModule configuration"):
        CSPNet(hidden_dim=64, num_layers=1, smooth=True, pred_type=True, pred_scalar=True)


def test_dropin_configs_compose():
    cfg = C.resolved(C.compose(EXAMPLE, "base", ["pipeline=predictor", "pipeline.train_path=/data/train.extxyz", "pipeline.properties=[density]",
                                                  "device=cuda:0"]))
    p = cfg.pipeline
    assert p._target_ == "pipeline.predictor.TrainPredictor" and p.train_path == "/data/train.extxyz" and list(p.properties) == ["density"]
    assert p.val_path is None and p.device == "cuda:0"
    t = p.train_cfg
    assert t.lr > 0 and t.epochs >= 1 and t.batch_size >= 1 and t.accum_steps == 1 and t.loss == "mse" and t.ema is None and t.lr_plateau is None
    assert p.model.hidden_dim % 64 == 0 and p.model.time_dim == 256
    r = C.resolved(C.compose(EXAMPLE, "base", ["reward=surrogate", "reward.model_path=/models/final"])).reward
    c = r.prop_cfg[0].calculator
    assert r._target_ == "rewards.reward.Reward" and c._target_ == "rewards.calculators.Surrogate" and c.model_path == "/models/final"
    assert c.task == r.prop_cfg[0].name == "density"
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        from pipeline.predictor import TrainPredictor
        from rewards.calculators import Surrogate
        from matinvent_amd import pipeline, rewards
        assert TrainPredictor is pipeline.TrainPredictor and hasattr(TrainPredictor, "run_rl") and Surrogate is rewards.Surrogate
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
    with pytest.raises(ValueError, match="train_path"):
        pipeline.TrainPredictor(None, "/tmp/x", ["density"])

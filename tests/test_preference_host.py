"""CPU-only checks of the preference fine-tune's host side (matinvent_amd.preference, pipeline.MatInventDPO): the pairing rule, the
refusals of dpo_step and of the pipeline before any device work, the epoch driver's route keys, and the drop-in config."""
import os
import sys

import numpy as np
import pytest

from matinvent_amd import config as C
from matinvent_amd import preference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "dropin", "configs")


def _rewards(n=23, seed=0):
    r = np.round(np.random.default_rng(seed).random(n), 2)
    r[3] = r[7]                                            # a tie: never a pair
    return r


def test_build_pairs_margin_order_and_no_duplicates():
    r = _rewards()
    for margin in (0.0, 0.25):
        p = preference.build_pairs(r, margin=margin)
        assert p.dtype == np.int64 and p.ndim == 2 and p.shape[1] == 2
        d = r[p[:, 0]] - r[p[:, 1]]
        assert np.all(d > 0) and np.all(d >= margin)
        assert len({tuple(x) for x in p.tolist()}) == len(p)
        assert p.tolist() == sorted(p.tolist())            # lexicographic (w, l)
        want = sum(1 for w in range(len(r)) for l in range(len(r)) if r[w] - r[l] > 0 and r[w] - r[l] >= margin)
        assert len(p) == want                              # everything returned when there is no cap
    assert [3, 7] not in p.tolist() and [7, 3] not in p.tolist()
    assert preference.build_pairs(np.full(5, 0.3)).shape == (0, 2)
    assert preference.build_pairs([]).shape == (0, 2)


def test_build_pairs_keys_and_winner_mask():
    r = _rewards()
    keys = ["NaCl" if i % 3 else "MgO" for i in range(len(r))]
    p = preference.build_pairs(r, keys=keys)
    assert len(p) and all(keys[w] == keys[l] for w, l in p.tolist())
    assert len(p) < len(preference.build_pairs(r))
    mask = np.zeros(len(r), dtype=bool)
    mask[np.argsort(-r)[:5]] = True
    q = preference.build_pairs(r, winners=mask)
    assert len(q) and all(mask[w] for w, _ in q.tolist()) and set(q[:, 0].tolist()) <= set(np.flatnonzero(mask).tolist())
    both = preference.build_pairs(r, keys=keys, winners=mask, margin=0.1)
    assert {tuple(x) for x in both.tolist()} <= {tuple(x) for x in p.tolist()} & {tuple(x) for x in q.tolist()}


def test_build_pairs_cap_is_a_deterministic_sorted_subset():
    r = _rewards()
    full = preference.build_pairs(r)
    assert np.array_equal(preference.build_pairs(r, max_pairs=len(full)), full)            # under the cap: all of them
    assert np.array_equal(preference.build_pairs(r, max_pairs=10 ** 6), full)
    a, b = preference.build_pairs(r, max_pairs=17, seed=4), preference.build_pairs(r, max_pairs=17, seed=4)
    assert a.shape == (17, 2) and np.array_equal(a, b)
    assert not np.array_equal(a, preference.build_pairs(r, max_pairs=17, seed=5))
    assert a.tolist() == sorted(a.tolist()) and len({tuple(x) for x in a.tolist()}) == 17
    assert {tuple(x) for x in a.tolist()} <= {tuple(x) for x in full.tolist()}
    idx = np.sort(np.random.default_rng(4).choice(len(full), 17, replace=False))           # the stated rule
    assert np.array_equal(a, full[idx])


class _Agent:
    device = "cpu"


@pytest.mark.parametrize("case", ["no beta", "no lr", "world", "mattergen", "empty", "range"])
def test_dpo_step_refusals_come_before_any_device_work(case, monkeypatch):
    cfg = dict(lr=1e-4, accum_steps=2, epochs=1, timesteps=2, dpo_beta=10.0)
    agent, pairs, data = _Agent(), [(0, 1)], [object(), object()]
    if case == "no beta":
        del cfg["dpo_beta"]
        with pytest.raises(KeyError, match="dpo_beta"):
            preference.dpo_step(agent, _Agent(), data, pairs, cfg)
        return
    if case == "no lr":
        del cfg["lr"]
        with pytest.raises(KeyError, match="lr"):
            preference.dpo_step(agent, _Agent(), data, pairs, cfg)
        return
    if case == "world":
        monkeypatch.setattr(preference, "rank_world", lambda: (0, 2))
    elif case == "mattergen":
        agent.collate = lambda *a: None
    elif case == "empty":
        pairs = np.zeros((0, 2), dtype=np.int64)
    else:
        pairs = [(0, 2)]
    match = {"world": "world_size", "mattergen": "MatterGen", "empty": "empty", "range": "outside"}[case]
    with pytest.raises(ValueError, match=match):
        preference.dpo_step(agent, _Agent(), data, pairs, cfg)


def test_epoch_stats_takes_a_routes_keys_and_keeps_ft_steps():
    from matinvent_amd import finetune
    a = [6.0, 12.0, 24.0]
    assert finetune._epoch_stats(a, 3, 4) == dict(loss=2.0, loss_diff=1.0, loss_kl=2.0)
    assert list(finetune._epoch_stats(a, 3, 4)) == ["loss", "loss_diff", "loss_kl"]
    assert finetune._epoch_stats(a, 3, 4, ("loss", "pref_acc", "margin")) == dict(loss=2.0, pref_acc=1.0, margin=2.0)


def test_dropin_dpo_config_composes():
    cfg = C.resolved(C.compose(EXAMPLE, "base", ["pipeline=mat_invent_dpo", "eval_size=6", "device=cuda:0"]))
    p = cfg.pipeline
    assert p._target_ == "pipeline.mat_invent_dpo.MatInventDPO"
    assert p.replay is True and p.div_filter is False and p.topk_ratio == 1.0
    ft = p.finetune_cfg
    assert ft.batch_size == 6 and ft.dpo_beta > 0 and ft.dpo_margin == 0.0 and ft.dpo_pairs is None and ft.dpo_within is None
    assert ft.accum_steps >= 1 and ft.epochs >= 1 and ft.timesteps >= 1
    assert C.merge(cfg.model.finetune_cfg, ft).lr == 0.0001
    text = open(os.path.join(EXAMPLE, "pipeline", "mat_invent_dpo.yaml")).read()
    assert "nobody has tuned" in text
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        from pipeline.mat_invent_dpo import MatInventDPO
        from matinvent_amd.pipeline import MatInvent
        assert issubclass(MatInventDPO, MatInvent)
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))


class _Suite:
    sample_cfg = C.create({"batch_size": 4, "num_batches": 1})
    finetune_cfg = C.create({"lr": 1e-4})


@pytest.mark.parametrize("case", ["mattergen", "world"])
def test_pipeline_refusals(case, monkeypatch, tmp_path):
    """MatInventDPO refuses the MatterGen suite and more than one GPU before it loads a model."""
    from matinvent_amd import pipeline
    from matinvent_amd.suite import MatterGenSuite
    kw = dict(rl_epoch=1, model_suite=_Suite(), reward=None, sample_cfg={}, finetune_cfg={}, save_dir=str(tmp_path), device="cpu")
    if case == "mattergen":
        kw["model_suite"] = MatterGenSuite.__new__(MatterGenSuite)
    else:
        monkeypatch.setattr(pipeline, "rank_world", lambda: (0, 2))
    with pytest.raises(ValueError, match={"mattergen": "MatterGen", "world": "world_size"}[case]):
        pipeline.MatInventDPO(**kw)

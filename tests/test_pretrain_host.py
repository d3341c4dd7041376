"""CPU-only checks of the supervised training's host side (matinvent_amd.pretrain, pipeline.Pretrain) and of tests/pretrain_ref64.py, the
float64 reference of the micro-step: the mini-batch plan and the time draws, the reference against an element-by-element evaluation at
the sizes the kernels loop over, the batch-size independence of evaluate's weighting, the refusals before any device work, the
boundary header with its ctypes table, the plateau scheduler, and the drop-in config."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from matinvent_amd import config as C
from matinvent_amd import pretrain
from tests import ft_ref64 as R
from tests import pretrain_ref64 as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "dropin", "configs")
LOOP_NA = [1, 2, 85, 86, 3, 171]


# ---- 1. the plan and the times --------------------------------------------------------------------------------------------------------

def test_batch_plan_is_a_reproducible_permutation_with_a_partial_last_batch():
    plan = pretrain.batch_plan(23, 5, epoch=0, seed=7)
    assert [len(b) for b in plan] == [5, 5, 5, 5, 3]
    assert sorted(i for b in plan for i in b) == list(range(23))
    assert plan == pretrain.batch_plan(23, 5, epoch=0, seed=7)
    assert plan != pretrain.batch_plan(23, 5, epoch=1, seed=7) and plan != pretrain.batch_plan(23, 5, epoch=0, seed=8)
    assert [i for b in plan for i in b] != list(range(23))
    assert pretrain.batch_plan(23, 5, epoch=3, seed=7, shuffle=False) == [list(range(s, min(23, s + 5))) for s in range(0, 23, 5)]
    assert pretrain.batch_plan(4, 100, 0, 0, shuffle=False) == [[0, 1, 2, 3]] and pretrain.batch_plan(0, 3, 0, 0) == []
    assert all(isinstance(i, int) for b in plan for i in b)
    with pytest.raises(ValueError, match="batch_size"):
        pretrain.batch_plan(5, 0, 0, 0)


def test_draw_times_stays_in_range_and_is_reproducible():
    t = pretrain.draw_times(4000, 10, epoch=2, step=3, seed=5)
    assert t.dtype == np.int32 and t.shape == (4000,) and int(t.min()) == 1 and int(t.max()) == 10
    assert np.array_equal(t, pretrain.draw_times(4000, 10, 2, 3, 5))
    for other in ((3, 3, 5), (2, 4, 5), (2, 3, 6)):
        assert not np.array_equal(t, pretrain.draw_times(4000, 10, *other))
    counts = np.bincount(t, minlength=11)[1:]
    assert abs(counts - 400).max() < 5 * np.sqrt(400 * 0.9)            # uniform over 1..T: every count within 5 sigma of its mean
    assert pretrain.draw_times(0, 10, 0, 0, 0).shape == (0,) and set(pretrain.draw_times(50, 1, 0, 0, 0).tolist()) == {1}


# ---- 2. the float64 reference against an element-by-element evaluation -------------------------------------------------------------

def _draws(na, seed):
    g = torch.Generator().manual_seed(seed)
    B, N = len(na), sum(na)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return (r(B, 3, 3), r(N, 3), r(N, 100)), (r(B, 3, 3), r(N, 3), r(N, 100))


def test_reference_matches_the_element_by_element_evaluation_at_the_loop_sizes():
    preds, targets = _draws(LOOP_NA, 0)
    B, N = len(LOOP_NA), sum(LOOP_NA)
    for b_global, n_global, accum in ((B, N, 1), (2 * B + 1, N + 11, 3)):
        st, parts, (sl, sx, stt) = PR.elementwise(preds, targets, PR.COSTS, LOOP_NA, b_global, n_global, accum)
        ref = PR.stats(preds, targets, PR.COSTS, b_global, n_global)
        assert float((ref - torch.tensor(st, dtype=torch.float64)).abs().max()) <= 1e-13 * float(ref.abs().max())
        P = PR.parts(preds, targets, LOOP_NA)
        assert float((P - torch.tensor(parts, dtype=torch.float64)).abs().max()) <= 1e-13 * float(P.abs().max())
        for s, e in zip(PR.seeds(preds, targets, PR.COSTS, b_global, n_global, accum), (sl, sx, stt)):
            e = torch.tensor(e, dtype=torch.float64).reshape(s.shape)
            assert float((s - e).abs().max()) <= 1e-15 * max(1.0, float(s.abs().max()))
    # the whole mini-batch: torch's three means, and the seeds are the autograd derivatives of loss / accum
    leaves = tuple(v.clone().requires_grad_(True) for v in preds)
    mse = torch.nn.functional.mse_loss
    three = [mse(p, t) for p, t in zip(leaves, targets)]
    loss = sum(c * v for c, v in zip(PR.COSTS, three))
    ref = PR.stats(preds, targets, PR.COSTS, B, N)
    assert float((ref - torch.stack([loss] + three).detach()).abs().max()) <= 1e-13 * float(ref.abs().max())
    for s, g in zip(PR.seeds(preds, targets, PR.COSTS, B, N, 3), torch.autograd.grad(loss / 3, leaves)):
        assert float((s - g).abs().max()) <= 1e-15 * max(1.0, float(g.abs().max()))


def test_every_atom_weighs_the_same_unlike_the_per_crystal_means_of_the_fine_tune_loss():
    """The 171-atom crystal beside the 1-atom one: with errors on the coordinates of ONE crystal only, the loss is that crystal's share of
    all atoms -- a per-crystal-mean loss (ft_ref64.loss_kl) gives every crystal the share 1 / B, off by n_b B / N."""
    B, N = len(LOOP_NA), sum(LOOP_NA)
    off = np.concatenate([[0], np.cumsum(LOOP_NA)])
    zero = lambda: (torch.zeros(B, 3, 3, dtype=torch.float64), torch.zeros(N, 3, dtype=torch.float64), torch.zeros(N, 100, dtype=torch.float64))
    for b in (0, 5):
        preds = zero()
        preds[1][off[b]:off[b + 1]] = 1.0
        got = float(PR.stats(preds, zero(), (0.0, 1.0, 0.0), B, N)[0])
        assert abs(got - LOOP_NA[b] / N) < 1e-15
        per_crystal = float(R.loss_kl(preds, preds, zero(), (0.0, 1.0, 0.0), LOOP_NA)[0].sum() / B)
        assert abs(per_crystal - 1 / B) < 1e-15 and abs(got / per_crystal - LOOP_NA[b] * B / N) < 1e-12


# ---- 3. evaluate's weighting --------------------------------------------------------------------------------------------------------

def test_evaluate_weighting_does_not_depend_on_batch_size():
    preds, targets = _draws(LOOP_NA, 1)
    B, N = len(LOOP_NA), sum(LOOP_NA)
    whole = PR.stats(preds, targets, PR.COSTS, B, N)
    for bs in (1, 2, 4, 5, 6, 100):
        got = PR.evaluate_ref(preds, targets, PR.COSTS, LOOP_NA, bs)
        assert float((got - whole).abs().max()) <= 1e-13 * float(whole.abs().max()), bs
    # the mean of the mini-batches' own losses is NOT the set's loss when their atom counts differ
    own = [PR.stats((preds[0][:3], preds[1][:88], preds[2][:88]), (targets[0][:3], targets[1][:88], targets[2][:88]), PR.COSTS, 3, 88),
           PR.stats((preds[0][3:], preds[1][88:], preds[2][88:]), (targets[0][3:], targets[1][88:], targets[2][88:]), PR.COSTS, 3, N - 88)]
    assert abs(float((own[0][2] + own[1][2]) / 2 - whole[2])) > 1e-6 * float(whole[2])


# ---- 4. the refusals ----------------------------------------------------------------------------------------------------------------

class _Model:
    device = "cpu"
    base = None


@pytest.mark.parametrize("case", ["respaced", "mattergen", "batch_size", "empty", "empty val", "no lr", "accum"])
def test_fit_refusals_come_before_any_device_work(case):
    cfg = dict(lr=1e-3, epochs=1, batch_size=2)
    model, data, kw = _Model(), [object(), object()], {}
    if case == "respaced":
        model.base = _Model()
    elif case == "mattergen":
        model.collate = lambda *a: None
    elif case == "batch_size":
        cfg["batch_size"] = 0
    elif case == "empty":
        data = []
    elif case == "empty val":
        kw["val_list"] = []
    elif case == "accum":
        cfg["accum_steps"] = 0
    else:
        del cfg["lr"]
        with pytest.raises(KeyError, match="lr"):
            pretrain.fit(model, data, cfg)
        return
    match = {"respaced": "respaced", "mattergen": "MatterGen", "batch_size": "batch_size", "empty": "empty training set",
             "empty val": "empty validation set", "accum": "accum_steps"}[case]
    with pytest.raises(ValueError, match=match):
        pretrain.fit(model, data, cfg, **kw)


def test_evaluate_and_train_step_refusals():
    view = _Model()
    view.base = _Model()
    for fn, args in ((pretrain.evaluate, (view, [object()], 2)), (pretrain.train_step, (view, None, [1]))):
        with pytest.raises(ValueError, match="respaced"):
            fn(*args)
    mg = _Model()
    mg.collate = lambda *a: None
    with pytest.raises(ValueError, match="MatterGen"):
        pretrain.evaluate(mg, [object()], 2)
    with pytest.raises(ValueError, match="batch_size"):
        pretrain.evaluate(_Model(), [object()], 0)
    with pytest.raises(ValueError, match="empty"):
        pretrain.evaluate(_Model(), [], 2)


def test_pipeline_refuses_the_mattergen_suite_and_a_missing_train_path(tmp_path):
    from matinvent_amd import pipeline
    from matinvent_amd.suite import MatterGenSuite
    with pytest.raises(ValueError, match="MatterGen"):
        pipeline.Pretrain(model_suite=MatterGenSuite.__new__(MatterGenSuite), train_path="x.extxyz", save_dir=str(tmp_path))

    class _Suite:
        finetune_cfg = C.create({"lr": 1e-4})
    with pytest.raises(ValueError, match="train_path"):
        pipeline.Pretrain(model_suite=_Suite(), train_path=None, save_dir=str(tmp_path))
    p = pipeline.Pretrain(model_suite=_Suite(), train_path="x.extxyz", save_dir=str(tmp_path), train_cfg={"lr": 1e-3, "epochs": 2, "batch_size": 4})
    assert p.train_cfg.lr == 1e-3 and p.train_cfg.batch_size == 4 and os.path.isdir(os.path.join(str(tmp_path), "models"))


def test_read_dataset_round_trips_write_extxyz(tmp_path):
    from matinvent_amd.data import CrystalData
    from matinvent_amd.pipeline import Pretrain
    from matinvent_amd.structure import write_extxyz
    g = torch.Generator().manual_seed(0)
    data = [CrystalData(torch.rand(n, 3, generator=g), torch.randint(1, 95, (n,), generator=g), 4 + 6 * torch.rand(1, 3, generator=g),
                        70 + 40 * torch.rand(1, 3, generator=g)) for n in (4, 1, 6)]
    path = write_extxyz(data, str(tmp_path / "set.extxyz"))
    back = Pretrain.read_dataset(path)
    assert [d.num_atoms for d in back] == [4, 1, 6]
    for a, b in zip(data, back):
        assert torch.equal(a.atom_types, b.atom_types) and b.lengths.shape == (1, 3) and b.angles.shape == (1, 3)
        d = (a.frac_coords - b.frac_coords).abs()
        assert float(torch.minimum(d, 1 - d).max()) < 1e-6 and float(b.frac_coords.min()) >= 0 and float(b.frac_coords.max()) < 1
        assert float((a.lengths - b.lengths).abs().max()) < 1e-5 and float((a.angles - b.angles).abs().max()) < 1e-4


# ---- 5. the header ------------------------------------------------------------------------------------------------------------------

def test_pretrain_header_is_exported_and_bound_in_its_own_table():
    from matinvent_amd import _lib
    from matinvent_amd.build import SOURCES, build
    from tests.header_util import declared_symbols
    names = declared_symbols("matinvent_hip_pretrain.h")
    assert sorted(names) == ["mi_pretrain_micro_step"] and "pretrain.hip" in SOURCES
    lib = ctypes.CDLL(build(verbose=False))
    assert all(hasattr(lib, n) for n in names)
    assert sorted(_lib.PRETRAIN_SIGNATURES) == sorted(names) and _lib.EXTENSION_SIGNATURES[-1] is _lib.PRETRAIN_SIGNATURES
    assert not set(names) & set(_lib.SIGNATURES)
    bound = _lib.load()
    for n in names:
        assert getattr(bound, n).argtypes == _lib.PRETRAIN_SIGNATURES[n][1] and getattr(bound, n).restype == _lib.PRETRAIN_SIGNATURES[n][0]
    assert len(_lib.PRETRAIN_SIGNATURES["mi_pretrain_micro_step"][1]) == 26
    # refused on the host, before any device work: null handles
    z = [None] * 10
    assert bound.mi_pretrain_micro_step(*z, 10, 0, 1, None, None, None, 1.0, 1.0, 20.0, 1, 1, 1, None, None, None, None) == _lib.MI_EINVAL
    assert b"null handle" in bound.mi_last_error()


# ---- 6. the plateau scheduler -------------------------------------------------------------------------------------------------------

def test_lr_plateau_follows_torchs_scheduler_on_a_recorded_loss_list():
    losses = [5.0, 4.0, 4.1, 4.2, 4.05, 3.0, 3.1, 3.2, 3.3, 3.4, 3.5, 3.6]
    spec = dict(factor=0.5, patience=2, min_lr=2e-4)
    mk = lambda: torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    o1, o2 = mk(), mk()
    s1 = pretrain.plateau_scheduler(o1, C.create(spec))
    s2 = torch.optim.lr_scheduler.ReduceLROnPlateau(o2, mode="min", factor=0.5, patience=2, min_lr=2e-4)
    assert isinstance(s1, torch.optim.lr_scheduler.ReduceLROnPlateau)
    seen = []
    for v in losses:
        seen.append(o1.param_groups[0]["lr"])
        s1.step(v)
        s2.step(v)
        assert o1.param_groups[0]["lr"] == o2.param_groups[0]["lr"]
    # worked by hand: best 4.0 at epoch 1, three epochs without improvement -> halved behind epoch 4; best 3.0 at epoch 5, halved behind
    # epoch 8 and again behind epoch 11, where min_lr = 2e-4 holds it
    assert seen == pytest.approx([1e-3] * 5 + [5e-4] * 4 + [2.5e-4] * 3) and o1.param_groups[0]["lr"] == pytest.approx(2e-4)
    assert pretrain.plateau_scheduler(mk(), None) is None
    with pytest.raises(ValueError, match="cooldown"):
        pretrain.plateau_scheduler(mk(), dict(factor=0.5, cooldown=1))


def test_fused_adam_is_a_torch_optimizer_the_scheduler_accepts():
    from matinvent_amd.optim import FusedAdam
    assert issubclass(FusedAdam, torch.optim.Optimizer)


# ---- the drop-in ----------------------------------------------------------------------------------------------------------------------

def test_dropin_pretrain_config_composes():
    cfg = C.resolved(C.compose(EXAMPLE, "base", ["pipeline=pretrain", "pipeline.train_path=/data/train.extxyz", "device=cuda:0"]))
    p = cfg.pipeline
    assert p._target_ == "pipeline.pretrain.Pretrain" and p.train_path == "/data/train.extxyz" and p.val_path is None
    t = p.train_cfg
    assert t.lr > 0 and t.epochs >= 1 and t.batch_size >= 1 and t.accum_steps == 1 and t.lr_plateau is None and t.max_grad_norm is None
    assert C.compose(EXAMPLE, "base", ["pipeline=pretrain"]).pipeline.train_path is None
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        from pipeline.pretrain import Pretrain
        from matinvent_amd import pipeline
        assert Pretrain is pipeline.Pretrain and hasattr(Pretrain, "run_rl")
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))


# ---- data parallel: the shards of a mini-batch ----------------------------------------------------------------------------------------

def test_shards_cover_a_mini_batch_with_its_offsets_and_counts():
    from types import SimpleNamespace
    items = [SimpleNamespace(num_atoms=n) for n in (4, 2, 6, 3, 1)]
    na = [d.num_atoms for d in items]
    noise = (torch.arange(5.0).view(5, 1, 1).expand(5, 3, 3), torch.arange(16.0).view(16, 1).expand(16, 3), torch.arange(16.0).view(16, 1).expand(16, 100))
    for world in (1, 2, 3, 7):
        seen, rows_l, rows_n = [], [], []
        for rank in range(world):
            own, offsets, b_glob, n_glob, rows = pretrain._shard(items, rank, world)
            assert (b_glob, n_glob) == (5, 16) and offsets == (sum(na[:rows[0]]), rows[0]) and own == items[rows[0]:rows[1]]
            seen += own
            nz = pretrain._slice_noise(noise, rows, na)
            rows_l += nz[0][:, 0, 0].tolist()
            rows_n += nz[1][:, 0].tolist()
            assert nz[2].shape == (sum(d.num_atoms for d in own), 100) and torch.equal(nz[1][:, 0], nz[2][:, 0])
        assert seen == items and rows_l == list(range(5)) and rows_n == list(range(16))   # every crystal and atom row once, in order
    assert pretrain._shard(items, 6, 7)[0] == [] and pretrain._slice_noise(None, (0, 1), na) is None

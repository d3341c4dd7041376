"""CPU-only checks of the weight average and of checkpoint / resume (include/matinvent_hip_ema.h; matinvent_amd.optim, .pretrain,
.pipeline): the header with its ctypes table, cfg.ema's parser, the decay schedule against hand-worked values and against
scripts/ema_host_check.cpp built with the host sanitizers, the meta refusals of a resume, the atomic save, and the pipeline's config."""
import ctypes as C
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from matinvent_amd import _lib
from matinvent_amd import config as CFG
from matinvent_amd.build import SOURCES, build
from tests.header_util import ROOT, declared_symbols

EXAMPLE = os.path.join(ROOT, "dropin", "configs")


# ---- the header -------------------------------------------------------------------------------------------------------------------------

def test_ema_header_is_exported_and_bound_in_its_own_table():
    names = declared_symbols("matinvent_hip_ema.h")
    assert names == ["mi_adam_step_ema"] and sorted(_lib.EMA_SIGNATURES) == names and "ema.hip" in SOURCES
    assert any(t is _lib.EMA_SIGNATURES for t in _lib.EXTENSION_SIGNATURES) and _lib.EXTENSION_SIGNATURES[-1] is _lib.PRETRAIN_SIGNATURES
    assert not set(names) & set(_lib.SIGNATURES)
    lib = C.CDLL(build(verbose=False))
    assert hasattr(lib, "mi_adam_step_ema")
    bound = _lib.load()
    res, args = _lib.EMA_SIGNATURES["mi_adam_step_ema"]
    assert bound.mi_adam_step_ema.restype == res and bound.mi_adam_step_ema.argtypes == args and len(args) == 16
    # the parent's three optimizer entries keep their signatures
    assert len(_lib.SIGNATURES["mi_adam_step"][1]) == 12 and len(_lib.OPTIM_SIGNATURES["mi_grad_norm"][1]) == 11
    assert len(_lib.OPTIM_SIGNATURES["mi_adam_step_guarded"][1]) == 11


def test_entry_refusals_come_before_anything_is_enqueued():
    """No GPU here: a call that got as far as a launch would fail with MI_EHIP, so MI_EINVAL / MI_OK show the host-side order."""
    f = _lib.load().mi_adam_step_ema
    p = C.c_void_p(4096)   # (never dereferenced on the host)

    def call(theta=p, grad=p, m=p, v=p, ema=p, n=8, step=1, decay=0.9, state=None):
        return f(theta, grad, m, v, ema, n, step, 1e-3, 0.9, 0.999, 1e-8, 1.0, decay, 1, state, None)
    for k in ("theta", "grad", "m", "v", "ema"):
        assert call(**{k: None}) == _lib.MI_EINVAL, k
    assert call(n=-1) == _lib.MI_EINVAL
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        assert call(decay=bad) == _lib.MI_EINVAL, bad
    assert call(step=0) == _lib.MI_EINVAL and b"step" in _lib.load().mi_last_error()
    assert call(n=0) == 0 and call(n=0, step=0, state=p) == 0 and call(n=0, decay=0.0) == 0   # (the guarded form ignores `step`)


# ---- cfg.ema ------------------------------------------------------------------------------------------------------------------------------

def test_parse_ema_and_its_refusals():
    from matinvent_amd.optim import parse_ema
    assert parse_ema(None) is None
    assert parse_ema(0.999) == dict(decay=0.999, warmup=True, validate=True) and parse_ema(0) == dict(decay=0.0, warmup=True, validate=True)
    assert parse_ema({"decay": 0.9}) == dict(decay=0.9, warmup=True, validate=True)
    assert parse_ema({"decay": 0.9, "warmup": False, "validate": None}) == dict(decay=0.9, warmup=False, validate=True)
    assert parse_ema(CFG.create({"decay": 0.5, "validate": False})) == dict(decay=0.5, warmup=True, validate=False)
    for bad in (1.0, -0.1, 1.5, float("nan"), True, "0.9", [0.9], {}, {"warmup": True}, {"decay": None}, {"decay": 1.0}, {"decay": "x"},
                {"decay": 0.9, "warmup": 1}, {"decay": 0.9, "validate": "yes"}, {"decay": 0.9, "rate": 2}):
        with pytest.raises(ValueError, match="ema"):
            parse_ema(bad)


def test_fit_refuses_a_bad_ema_before_any_device_work():
    from matinvent_amd import pretrain
    m = SimpleNamespace(base=None)   # (no decoder, no device: reaching either would be an AttributeError)
    with pytest.raises(ValueError, match="ema"):
        pretrain.fit(m, [object()], dict(lr=1e-3, epochs=1, batch_size=2, ema=1.0))


# ---- the decay schedule -----------------------------------------------------------------------------------------------------------------

def test_decay_schedule_hand_worked_values():
    from matinvent_amd.optim import ema_decay_at
    f32 = lambda x: float(np.float32(x))
    assert ema_decay_at(0.999, True, 1) == f32(2 / 11) and ema_decay_at(0.999, True, 10) == f32(11 / 20)
    # (1 + s) / (10 + s) >= 0.999  <=>  0.001 s >= 8.99  <=>  s >= 8990: there the warm-up's 8991 / 9000 and the decay round to one float
    takes_over = next(s for s in range(1, 20000) if ema_decay_at(0.999, True, s) == f32(0.999))
    assert takes_over == 8990
    assert ema_decay_at(0.999, True, 8989) == f32(8990 / 8999) < f32(0.999)
    assert all(ema_decay_at(0.999, True, s) == f32(0.999) for s in (8991, 10 ** 6, 2 ** 32 - 1))
    assert ema_decay_at(0.9, True, 79) == f32(80 / 89) < f32(0.9) and ema_decay_at(0.9, True, 80) == f32(0.9)   # 81 / 90 = 0.9
    # warm-up off: the decay itself, from the first step on
    assert all(ema_decay_at(0.999, False, s) == f32(0.999) for s in (1, 10, 8989)) and ema_decay_at(0.0, True, 5) == 0.0


def test_decay_schedule_against_the_host_program_under_the_sanitizers(tmp_path):
    """scripts/ema_host_check.cpp compiles csrc/ema_decay.h -- the text the entry's host side and the guarded kernel's waves run -- with
    -fsanitize=address,undefined; its printed bits equal numpy's for warm-up on and off."""
    from matinvent_amd.optim import ema_decay_at
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "ema_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "scripts", "ema_host_check.cpp"), "-o", exe], check=True)
    steps = [0, 1, 2, 3, 9, 10, 11, 80, 81, 82, 999, 8989, 8990, 8991, 123456, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]
    for decay in (0.999, 0.9, 0.9999, 0.5, 0.0):
        for warmup in (1, 0):
            r = subprocess.run([exe, repr(decay), str(warmup)] + [str(s) for s in steps], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            assert r.returncode == 0, r.stdout + r.stderr
            rows = [ln.split() for ln in r.stdout.splitlines()]
            assert [int(x[0]) for x in rows] == steps
            want = [np.float32(ema_decay_at(decay, bool(warmup), s)).view(np.uint32) for s in steps]
            assert [int(x[1], 16) for x in rows] == [int(w) for w in want], (decay, warmup, r.stdout)
    assert subprocess.run([exe, "0.9"], stderr=subprocess.PIPE).returncode == 2


# ---- resume: the meta -------------------------------------------------------------------------------------------------------------------

def _meta(**kw):
    m = dict(seed=3, batch_size=4, accum_steps=3, shuffle=True, n_train=6, n_val=4, world_size=1, T=1000, numel=1234, max_grad_norm=0.5,
             skip_nonfinite=True, ema_decay=0.9, ema_warmup=True, ema_validate=True, lr_plateau=True)
    m.update(kw)
    return m


def test_every_meta_key_mismatch_raises_and_names_itself():
    from matinvent_amd import pretrain
    assert set(_meta()) == set(pretrain.META_KEYS)
    pretrain.check_meta(_meta(), _meta())
    other = dict(seed=4, batch_size=3, accum_steps=1, shuffle=False, n_train=7, n_val=0, world_size=2, T=20, numel=1235, max_grad_norm=None,
                 skip_nonfinite=False, ema_decay=None, ema_warmup=False, ema_validate=False, lr_plateau=False)
    assert set(other) == set(pretrain.META_KEYS)
    for k, v in other.items():
        with pytest.raises(ValueError, match=rf"\b{k} = "):
            pretrain.check_meta(_meta(), _meta(**{k: v}))
    saved = _meta()
    del saved["world_size"]
    with pytest.raises(ValueError, match="world_size"):
        pretrain.check_meta(saved, _meta())


# ---- the atomic save --------------------------------------------------------------------------------------------------------------------

def test_save_training_state_replaces_atomically_and_leaves_no_temporary_file(tmp_path):
    from matinvent_amd import pretrain
    path = str(tmp_path / "train_state.ckpt")
    first = dict(theta=torch.arange(5.0), epoch=2, history=[{"train_loss": 1.5}], meta=_meta())
    assert pretrain.save_training_state(path, first) == path and os.listdir(tmp_path) == ["train_state.ckpt"]
    size = os.path.getsize(path)

    def dies_half_way(obj, f):   # a writer that is killed in the middle of the file
        f.write(b"\0" * (size // 2))
        f.flush()
        raise KeyboardInterrupt("killed")
    with pytest.raises(KeyboardInterrupt):
        pretrain.save_training_state(path, dict(first, epoch=3), _save=dies_half_way)
    assert os.listdir(tmp_path) == ["train_state.ckpt"] and os.path.getsize(path) == size
    back = pretrain.load_training_state(path)
    assert back["epoch"] == 2 and torch.equal(back["theta"], first["theta"]) and back["history"] == first["history"] and back["meta"] == first["meta"]
    # ... and a write that completes does replace it
    pretrain.save_training_state(path, dict(first, epoch=3))
    assert pretrain.load_training_state(path)["epoch"] == 3 and os.listdir(tmp_path) == ["train_state.ckpt"]


# ---- the pipeline and the drop-in -------------------------------------------------------------------------------------------------------

def test_pretrain_merges_ema_and_resume_from(tmp_path):
    from matinvent_amd import pipeline

    class _Suite:
        finetune_cfg = CFG.create({"lr": 1e-4, "ema": 0.5})
    p = pipeline.Pretrain(model_suite=_Suite(), train_path="x.extxyz", save_dir=str(tmp_path), train_cfg={"epochs": 2, "batch_size": 4, "ema": {"decay": 0.99}},
                          resume_from=str(tmp_path / "models" / "epoch_0001"))
    assert p.train_cfg.ema.decay == 0.99 and p.train_cfg.lr == 1e-4 and p.resume_from.endswith("epoch_0001")
    q = pipeline.Pretrain(model_suite=_Suite(), train_path="x.extxyz", save_dir=str(tmp_path), train_cfg={"epochs": 2, "batch_size": 4})
    assert q.train_cfg.ema == 0.5 and q.resume_from is None   # (the suite's finetune_cfg underneath)
    cfg = CFG.resolved(CFG.compose(EXAMPLE, "base", ["pipeline=pretrain", "pipeline.train_path=/data/t.extxyz", "device=cuda:0"]))
    assert cfg.pipeline.resume_from is None and cfg.pipeline.train_cfg.ema is None
    cfg = CFG.resolved(CFG.compose(EXAMPLE, "base", ["pipeline=pretrain", "+pipeline.train_cfg.ema=0.9", "pipeline.resume_from=/r/models/epoch_0001"]))
    assert cfg.pipeline.train_cfg.ema == 0.9 and cfg.pipeline.resume_from == "/r/models/epoch_0001"

"""CPU checks of the relaxation on a learned energy that need no GPU (matinvent_amd.relax, include/matinvent_hip_relax.h,
matinvent_amd/csrc/relax_fire.h): the header, its table and the build list; the host check compiled with the host sanitizers
and run; the reference's own consistency -- its forces against a finite difference of the synthetic energy, every branch taken and no
decision tied on the cases tests/test_gpu_relax.py runs; Relaxer's refusals by name; the pipelines' handling of the key; the drop-in
config."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from matinvent_amd import _lib, config as C, predictor as PR, relax as RX
from tests import relax_ref64 as R
from tests.header_util import ROOT, declared_symbols

EXAMPLE = os.path.join(ROOT, "dropin", "configs")
# the cases of tests/test_gpu_relax.py: (atom counts, seed of make_case); 40 consecutive steps, with and without relax_cell
LOOP_NA = [1, 2, 171, 20, 3]
GRID_NA = [1 + (i * 7 + i // 3) % 3 for i in range(300)]
CASES = dict(loop=(LOOP_NA, 5), grid=(GRID_NA, 34))
STEPS = 40
TEST_PARAMS = dict(dt_max=0.25)   # (the cap is reached within the run: dt halves at step 0 and grows by 1.1 per step past n_min)


def _predictor(names=("energy", "gap"), **kw):
    return PR.PropertyPredictor(list(names), hidden_dim=64, num_layers=1, time_dim=256, num_freqs=8, device="cpu", seed=1, **kw)


def test_header_table_and_build_list():
    from matinvent_amd.build import SOURCES
    names = sorted(declared_symbols("matinvent_hip_relax.h"))
    assert names == ["mi_relax_init", "mi_relax_run", "mi_relax_step"]
    assert sorted(_lib.RELAX_SIGNATURES) == names and any(t is _lib.RELAX_SIGNATURES for t in _lib.EXTENSION_SIGNATURES)
    assert "relax.hip" in SOURCES
    head = open(os.path.join(ROOT, "include", "matinvent_hip_relax.h")).read()
    text = open(os.path.join(ROOT, "matinvent_amd", "csrc", "relax_fire.h")).read()
    for k, name in enumerate(("ACTIVE", "CONVERGED", "FAILED", "EXHAUSTED")):
        assert f"#define MI_RELAX_{name} {k}" in head and f"RELAX_{name} = {k}" in text
    assert (_lib.RELAX_ACTIVE, _lib.RELAX_CONVERGED, _lib.RELAX_FAILED, _lib.RELAX_EXHAUSTED) == (R.ACTIVE, R.CONVERGED, R.FAILED, R.EXHAUSTED) == (0, 1, 2, 3)
    assert "#define MI_RELAX_NF 6" in head and "#define MI_RELAX_NI 3" in head and (_lib.RELAX_NF, _lib.RELAX_NI) == (R.NF, R.NI) == (6, 3)
    assert "fp contract(off)" in text
    for f in ("relax_host_check.cpp", "relax_timing.py"):
        assert os.path.exists(os.path.join(ROOT, "scripts", f))
    # the parameter block is the header's struct, field for field
    fields = [k for k, _ in _lib.RelaxParams._fields_]
    assert fields == ["dt", "dt_max", "maxstep", "f_inc", "f_dec", "a_start", "f_a", "fmax", "scale", "cell_factor", "det_min", "n_min", "relax_cell", "per_atom"]
    body = head[head.index("typedef struct"):head.index("} mi_relax_params")]
    at = -1
    for k in fields:
        nxt = body.index(f" {k}", at + 1)
        assert nxt > at, k
        at = nxt
    # the entries bind, and their host-only refusals answer without a GPU
    import ctypes
    lib = _lib.load()
    ok = RX.Relaxer(_predictor(), "energy").params()
    assert lib.mi_relax_init(None, ctypes.byref(ok), 1, 0, *([None] * 6)) == _lib.MI_EINVAL and b"null handle" in lib.mi_last_error()
    assert lib.mi_relax_step(None, ctypes.byref(ok), 1, 0, *([None] * 10)) == _lib.MI_EINVAL
    assert lib.mi_relax_run(None, None, ctypes.byref(ok), *([None] * 6), 1, 0, *([None] * 8), 1, 1, None) == _lib.MI_EINVAL


def test_host_check_under_the_host_sanitizers(tmp_path):
    """scripts/relax_host_check.cpp: csrc/relax_fire.h -- what relax_step_kernel calls -- against a plain loop, bit for bit, with every
    branch taken; built with AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "relax_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "scripts", "relax_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, "300", "1"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "300 rounds" in r.stdout and " 0 mismatches" in r.stdout


def test_the_tree_and_the_inverse():
    rng = np.random.default_rng(0)
    for Rr in (1, 2, 3, 5, 8, 23, 174):
        a = rng.standard_normal((4, Rr))
        assert np.allclose(R.tree_sum(a), a.sum(axis=1), rtol=0, atol=1e-12)
    assert [R.tree_half(k) for k in (1, 2, 3, 4, 5, 174)] == [0, 1, 2, 2, 4, 128]
    L = np.eye(3)[None] * 5.0 + rng.uniform(-1, 1, (6, 3, 3))
    det, Li = R.inv3(L, np.float64)
    assert np.allclose(det, np.linalg.det(L)) and np.allclose(Li, np.linalg.inv(L), atol=1e-13)


def test_the_reference_forces_are_minus_the_energy_gradient():
    """F = -g L^-T is -dE/d(cart) and F_L = -g_lat / c is -dE/dL / c: central differences of the synthetic energy in float64, and the first
    step from v = 0 moves straight along the force and lowers the energy."""
    case = R.make_case([3, 2, 4], seed=11)
    na, spec = case["na"], case["spec"]
    x, L = case["frac"].astype(np.float64), case["lat"].astype(np.float64)
    E0, gx, gl = R.harmonic(na, spec, x, L)
    h = 1e-6
    rng = np.random.default_rng(2)
    for _ in range(6):
        i, d = int(rng.integers(len(x))), int(rng.integers(3))
        xp, xm = x.copy(), x.copy()
        xp[i, d] += h
        xm[i, d] -= h
        fd = (R.harmonic(na, spec, xp, L)[0].sum() - R.harmonic(na, spec, xm, L)[0].sum()) / (2 * h)
        assert abs(fd - gx[i, d]) <= 1e-6 * np.abs(gx).max()
        b, q, k = int(rng.integers(3)), int(rng.integers(3)), int(rng.integers(3))
        Lp, Lm = L.copy(), L.copy()
        Lp[b, q, k] += h
        Lm[b, q, k] -= h
        fd = (R.harmonic(na, spec, x, Lp)[0].sum() - R.harmonic(na, spec, x, Lm)[0].sum()) / (2 * h)
        assert abs(fd - gl[b, q, k]) <= 1e-6 * np.abs(gl).max()
    for cell in (0, 1):
        prm = R.params(relax_cell=cell, fmax=1e-6, maxstep=10.0, dt=0.02)
        st = R.new_state(na, x, L, prm, np.float64)
        rec = R.fire_step(na, prm, st, gx, gl, E0)
        assert rec["moved"].all() and not rec["positive"].any() and np.all(st["fs"][:, R.F_DT] == prm["dt"] * prm["f_dec"])
        E1 = R.harmonic(na, spec, st["frac"], st["lat"])[0]
        assert np.all(E1 < E0)
        assert (not cell) == np.array_equal(st["lat"], L)
        # a frozen crystal keeps every bit; a non-finite gradient fails the crystal and writes nothing else
        st2 = R.new_state(na, x, L, prm, np.float64)
        st2["is_"][1, R.I_STATUS] = R.CONVERGED
        bad = gx.copy()
        bad[0, 1] = np.nan
        R.fire_step(na, prm, st2, bad, gl, E0)
        assert st2["is_"][:, R.I_STATUS].tolist() == [R.FAILED, R.CONVERGED, R.ACTIVE]
        assert np.array_equal(st2["frac"][:5], x[:5]) and np.array_equal(st2["lat"][:2], L[:2]) and not st2["vel_x"][:5].any()
        assert np.array_equal(st2["frac"][5:], st["frac"][5:])


@pytest.mark.parametrize("name", ["loop", "grid"])
@pytest.mark.parametrize("cell", [0, 1])
def test_the_reference_run_takes_every_branch_and_ties_nowhere(name, cell):
    """What tests/test_gpu_relax.py demands of its inputs, checked here first: on the float64 reference every decision's margin lies
    outside TIE, the float32 restatement takes the same decisions, and the branches occur."""
    na, seed = CASES[name]
    case = R.make_case(na, seed)
    prm = R.params(relax_cell=cell, **TEST_PARAMS)
    s64, r64 = R.run(case, prm, STEPS, np.float64)
    rep = R.branch_report(case, r64, s64)
    assert min(rep["m_P"], rep["m_fmax"], rep["m_clamp"]) > R.TIE, rep
    assert rep["nonpositive"] and rep["grew"] and rep["converged_mid_run"] and rep["one_atom_at_step_0"], rep
    if name == "loop":   # (the stiff 171-atom crystal and the two-atom one: the clamp and the cap)
        assert rep["capped"] and rep["clamped"], rep
    s32, _ = R.run(case, prm, STEPS, np.float32)
    dev = R.deviation(s32, s64)
    assert dev["is_equal"], "the float32 restatement took another decision than float64"
    assert max(dev["frac"], dev["dt"]) < 1e-4 and all(np.isfinite(v) for v in dev.values())
    assert np.isin(s64["is_"][:, R.I_STATUS], (R.ACTIVE, R.CONVERGED)).all()


def test_relaxer_refuses_by_name():
    p = _predictor()
    r = RX.Relaxer(p, "gap", steps=7, relax_cell=False, per_atom=False, cell_factor=2.0, dt_max=0.5)
    assert (r.p, r.steps, r.relax_cell, r.per_atom, r.cell_factor, r.fire["dt_max"], r.fire["n_min"], r.check_every) == (1, 7, False, False, 2.0, 0.5, 5, 0)
    prm = r.params()
    assert (prm.relax_cell, prm.per_atom, prm.n_min) == (0, 0, 5) and prm.cell_factor == 2.0 and prm.scale == np.float32(p.normalizer.std[1])
    assert RX.Relaxer(p, "energy").params().cell_factor == 0.0   # (the crystal's atom count)
    assert {k: RX.FIRE_DEFAULTS[k] for k in RX.FIRE_DEFAULTS} == {k: R.DEFAULTS[k] for k in RX.FIRE_DEFAULTS}
    with pytest.raises(ValueError, match="knn-style"):
        RX.Relaxer(_predictor(edge_style="knn"), "gap")
    for kw, match in ((dict(task="volume"), "not a property"), (dict(task="gap", steps=-1), "steps"), (dict(task="gap", fmax=0.0), "fmax"),
                      (dict(task="gap", fmax=float("nan")), "fmax"), (dict(task="gap", dt=float("inf")), "dt"), (dict(task="gap", maxstep=-0.1), "maxstep"),
                      (dict(task="gap", n_min=-1), "n_min"), (dict(task="gap", check_every=-2), "check_every"), (dict(task="gap", batch_size=0), "batch_size"),
                      (dict(task="gap", cell_factor=0.0), "cell_factor"), (dict(task="gap", cell_factor=float("inf")), "cell_factor"),
                      (dict(task="gap", det_min=0.0), "det_min"), (dict(task="gap", f_up=2.0), "unknown keywords")):
        with pytest.raises(ValueError, match=match):
            RX.Relaxer(p, **kw)
    with pytest.raises(ValueError, match="model_path"):
        RX.Relaxer.from_config({"task": "gap"})
    assert RX.Relaxer.from_config(None) is None and RX.Relaxer.from_config(r) is r


def test_relax_records_without_a_record_to_run_needs_no_device():
    """Order and length survive; a record the network cannot take comes back as it was with energy NaN."""
    from matinvent_amd.data import SimpleStructure
    r = RX.Relaxer(_predictor(), "energy")
    bad = [SimpleStructure([4.0, 4.0, 4.0], [90.0, 90.0, 90.0], [], np.zeros((0, 3))),
           SimpleStructure([4.0, 4.0, 4.0], [90.0, 90.0, 90.0], [120], np.zeros((1, 3))),
           SimpleStructure([4.0, 4.0, float("nan")], [90.0, 90.0, 90.0], [3], np.zeros((1, 3)))]
    out, e = r(bad, None)
    assert len(out) == 3 and all(a is b for a, b in zip(out, bad)) and e.dtype == np.float64 and np.isnan(e).all()
    assert r.last_info["status"].tolist() == [-1, -1, -1]
    assert RX.log_metrics(r, e) == dict(relax_converged=0, relax_failed=3, relax_steps_mean=pytest.approx(float("nan"), nan_ok=True),
                                        relax_de_mean=pytest.approx(float("nan"), nan_ok=True))
    le, an = RX._lengths_angles(np.array([[3.0, 0, 0], [0, 4.0, 0], [0, 3.0, 3.0]]))
    assert np.allclose(le, [3, 4, 18 ** 0.5]) and np.allclose(an, [45.0, 90.0, 90.0])


def test_the_pipelines_take_the_key(tmp_path):
    """relax_step hands (strucs, xyz_path) to the callable and its energies on; anything else under the key is refused by name; without
    the key nothing is called."""
    from matinvent_amd import pipeline
    from matinvent_amd.suite import DiffCSPSuite
    suite = DiffCSPSuite("diffcsp", {"batch_size": 4, "num_batches": 1}, {}, device="cpu")
    seen = []

    def opt(strucs, xyz_path=None):
        seen.append((list(strucs), xyz_path))
        return [s.upper() for s in strucs], np.array([1.5, float("nan")])

    rl = pipeline.ReinL(rl_epoch=1, model_suite=suite, reward=None, sample_cfg={"mlip_opt": opt}, finetune_cfg={}, save_dir=str(tmp_path), save_freq=1, device="cpu")
    strucs, energies, log = rl.relax_step(["a", "b"], "/x.extxyz")
    assert strucs == ["A", "B"] and seen == [(["a", "b"], "/x.extxyz")] and energies[0] == 1.5
    assert set(log) == {"relax_converged", "relax_failed", "relax_steps_mean", "relax_de_mean"} and log["relax_failed"] == 1
    plain = pipeline.ReinL(rl_epoch=1, model_suite=suite, reward=None, sample_cfg={}, finetune_cfg={}, save_dir=str(tmp_path), save_freq=1, device="cpu")
    assert plain.relax_step(["a"]) == (["a"], None, {})
    wrong = pipeline.ReinL(rl_epoch=1, model_suite=suite, reward=None, sample_cfg={"mlip_opt": {"task": "energy"}}, finetune_cfg={}, save_dir=str(tmp_path),
                           save_freq=1, device="cpu")
    with pytest.raises(ValueError, match="mlip_opt takes a callable"):
        wrong.relax_step(["a"])
    short = pipeline.ReinL(rl_epoch=1, model_suite=suite, reward=None, sample_cfg={"mlip_opt": lambda s, p=None: (s, [])}, finetune_cfg={},
                           save_dir=str(tmp_path), save_freq=1, device="cpu")
    with pytest.raises(ValueError, match="0 energies for 1 samples"):
        short.relax_step(["a"])


def test_dropin_config_composes():
    for where in ("sample_cfg.mlip_opt", "pipeline.sample_cfg.mlip_opt"):   # (pipeline.sample_cfg only points at sample_cfg)
        cfg = C.resolved(C.compose(EXAMPLE, "base", [f"+relax@{where}=surrogate", "sample_cfg.mlip_opt.model_path=/models/energy", "sample_cfg.mlip_opt.steps=20"]))
        for m in (cfg.sample_cfg.mlip_opt, cfg.pipeline.sample_cfg.mlip_opt):
            assert m["_target_"] == "pipeline.relax.SurrogateRelaxer" and m.model_path == "/models/energy" and m.steps == 20 and m.task == "energy"
            assert m.fmax == 0.1 and m.relax_cell is True and m.per_atom is True and m.cell_factor is None and m.check_every == 0 and m.batch_size == 64
    plain = C.resolved(C.compose(EXAMPLE, "base", []))
    assert "mlip_opt" not in plain.sample_cfg
    import sys
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        from pipeline.relax import SurrogateRelaxer
        assert issubclass(SurrogateRelaxer, RX.Relaxer)
        with pytest.raises(ValueError, match="model_path"):
            SurrogateRelaxer(task="energy")
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
